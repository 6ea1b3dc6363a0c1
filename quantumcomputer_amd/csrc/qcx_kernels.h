// qcx_kernels.h -- hand-written gfx950 (CDNA4) kernels for the gate-application
// path of qc_shor.c.  HBM-bound streaming kernels on the in-place amplitude
// vector; wave64 everywhere.  No matrix is built and no mat-vec is run: each
// kernel computes, per amplitude, exactly the sums the reference's COO
// mat-vec (Q:396-413) would have produced for that gate, in the same order
// and with the same roundings (compile with -ffp-contract=off).
//
// Bit-exactness notes (proved against the oracle in tests/):
//   reference output  = 0 + term0 (+ term1), term = (mr*cr)-(mi*ci) with mi = 0
//   kernel output     = (t0 (+|-) t1) + 0.0
// identical for every finite input, zero signs included: the only effect of
// the reference's "0 +" and "- 0*x" is to turn a -0 result into +0, which the
// trailing "+ 0.0" reproduces (it is not foldable under IEEE rules).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace qcx {

typedef double amp_t __attribute__((ext_vector_type(2)));   // (re, im): one 16-B global access

#define QCX_SQRT1_2 0.70710678118654752440   /* M_SQRT1_2, Q:210-213 */

__device__ __forceinline__ uint64_t insert_zero(uint64_t p, unsigned b)
{
    const uint64_t low = ((uint64_t)1 << b) - 1;
    return ((p & ~low) << 1) | (p & low);
}

template <bool NT> __device__ __forceinline__ amp_t ld(const amp_t *p)
{
    if (NT) return __builtin_nontemporal_load(p);
    return *p;
}
template <bool NT> __device__ __forceinline__ void st(amp_t *p, amp_t v)
{
    if (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// The reference's mat-vec on one stored triplet (Q:396-413): the matrix entry (mr, mi) times the amplitude x -- four products
// and two sums, each rounded on its own (no FMA: this file is compiled with fp contraction off), nothing skipped where a
// component is zero.  Every general gate (K9, K12, K13, K15) forms its products here and nowhere else.
struct q_mul {
    double mr, mi;
    amp_t x;
    __device__ __forceinline__ q_mul(double mr_, double mi_, amp_t x_) : mr(mr_), mi(mi_), x(x_) {}
    __device__ __forceinline__ double re() const { return (mr * x.x) - (mi * x.y); }      // Q:409
    __device__ __forceinline__ double im() const { return (mr * x.y) + (mi * x.x); }      // Q:412
};

// One row of that mat-vec: the reference's accumulator starts at (+0, +0) and adds the row's products in the order given
// (ascending column), ((0 + p0) + p1) + ...  The "0 +" cannot be dropped: it turns a -0 first product into +0, which is what
// the reference stores, and changes no other value; IEEE rules do not let a compiler fold it either (0 + -0 = +0 is not the
// identity), and the build tests look for the surviving v_add_f64 with a literal 0.  q_row() alone is the empty sum (+0, +0).
// (Each component's chain is formed in one piece, its products where they are added: few values are live at a time.)
template <typename... P> __device__ __forceinline__ amp_t q_row(const P &... p)
{
    amp_t acc;
    acc.x = 0.0; ((acc.x = acc.x + p.re()), ...);
    acc.y = 0.0; ((acc.y = acc.y + p.im()), ...);
    return acc;
}

// The interleaved block -> tile map of the general gates (K12, K13): with slog > 0 the 2^glog tiles are dealt as 2^slog
// streams, so blocks b, b + 2^slog, ... walk one contiguous region (speed only, any placement is correct).  K1b and K2 keep
// this line spelled out: their prologues are scheduled around it and they are the benchmark's kernels.
__device__ __forceinline__ uint64_t stream_tile(unsigned glog, unsigned slog)
{
    uint64_t tile = blockIdx.x;
    if (slog) tile = ((uint64_t)(blockIdx.x & ((1u << slog) - 1u)) << (glog - slog)) | (blockIdx.x >> slog);
    return tile;
}

// one Hadamard butterfly: a = amplitude with target bit 0, b = with target bit 1
__device__ __forceinline__ void h_butterfly(amp_t &a, amp_t &b)
{
    const double s = QCX_SQRT1_2;
    const double t0r = s * a.x, t0i = s * a.y, t1r = s * b.x, t1i = s * b.y;
    a.x = (t0r + t1r) + 0.0;  a.y = (t0i + t1i) + 0.0;
    b.x = (t0r - t1r) + 0.0;  b.y = (t0i - t1i) + 0.0;
}

// ---------------------------------------------------------------------------
// K1a  Hadamard, pair form, any target qubit.  Thread p owns the pair
// (i0, i0 | 2^q) with i0 = p with a zero inserted at bit q.  For q >= 6 both
// streams are 1-KiB-per-wave-instruction coalesced; below that the two loads of
// a wave interleave inside one 2-KiB window.  PPT pairs per thread are loaded
// before any is stored (2*PPT independent 16-B loads in flight per lane).
// ---------------------------------------------------------------------------
template <int PPT, bool NTL, bool NTS, bool WC, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_h_pair(amp_t *__restrict__ amp, unsigned q, uint64_t npairs,
                                                    unsigned glog, unsigned slog)
{
    const uint64_t low = ((uint64_t)1 << q) - 1, bit = (uint64_t)1 << q;
    const uint64_t step = (uint64_t)gridDim.x * (BLOCK * PPT);
    // WC: a wave's PPT loads are consecutive 64-pair runs (per-wave contiguous); otherwise the
    // block's waves interleave (k-th load of the block covers BLOCK consecutive pairs)
    const unsigned toff = WC ? ((threadIdx.x >> 6) * (64 * PPT) + (threadIdx.x & 63u)) : threadIdx.x;
    constexpr unsigned kstride = WC ? 64 : BLOCK;
    // block -> tile map: with slog > 0 the 2^glog tiles are dealt as 2^slog interleaved streams, so
    // blocks b, b + 2^slog, ... walk one contiguous region (slog = 3: one stream per XCD under the
    // round-robin block placement; speed only, any placement is correct)
    uint64_t tile0 = blockIdx.x;
    if (slog & 0xffu) {
        // streams; optional skew (slog >> 8): stream j walks its segment rotated by j * skew tiles, so that the
        // concurrently active windows are NOT a power-of-two distance apart
        const unsigned sl = slog & 0xffu, skew = slog >> 8;
        const uint64_t j = blockIdx.x & ((1u << sl) - 1u), pos = blockIdx.x >> sl, seg = (uint64_t)1 << (glog - sl);
        tile0 = (j << (glog - sl)) | ((pos + j * skew) & (seg - 1));
    }
    for (uint64_t base = tile0 * (BLOCK * PPT); base < npairs; base += step) {
        amp_t a[PPT], b[PPT];
        uint64_t i0[PPT];
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            const uint64_t p = base + (uint64_t)k * kstride + toff;
            i0[k] = ((p & ~low) << 1) | (p & low);
            if (p < npairs) { a[k] = ld<NTL>(amp + i0[k]); b[k] = ld<NTL>(amp + i0[k] + bit); }
        }
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            const uint64_t p = base + (uint64_t)k * kstride + toff;
            if (p < npairs) {
                h_butterfly(a[k], b[k]);
                st<NTS>(amp + i0[k], a[k]);
                st<NTS>(amp + i0[k] + bit, b[k]);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// K1b  Hadamard, wave-tile form for low target qubits (q < 6 + log2 R).
// A wave owns 64*R consecutive amplitudes as R registers x 64 lanes, every
// load/store a fully coalesced 1 KiB.  Partners sit in another lane (q < 6:
// wavefront xor-shuffle butterfly) or in another register of the same lane.
// ---------------------------------------------------------------------------
__device__ __forceinline__ amp_t shfl_xor_amp(amp_t v, int lane_mask)
{
    amp_t r;
    r.x = __shfl_xor(v.x, lane_mask, 64);
    r.y = __shfl_xor(v.y, lane_mask, 64);
    return r;
}

template <int Q, int R>
__device__ __forceinline__ void h_wave_tile(amp_t (&r)[R], unsigned lane)
{
    const double s = QCX_SQRT1_2;
    if constexpr (Q < 6) {
        const bool upper = (lane >> Q) & 1u;
#pragma unroll
        for (int k = 0; k < R; k++) {
            amp_t t; t.x = s * r[k].x; t.y = s * r[k].y;
            const amp_t o = shfl_xor_amp(t, 1 << Q);
            // lower lane: t + o ; upper lane: o - t   (o is the bit-0 partner's product)
            r[k].x = (upper ? (o.x - t.x) : (t.x + o.x)) + 0.0;
            r[k].y = (upper ? (o.y - t.y) : (t.y + o.y)) + 0.0;
        }
    } else {
        constexpr int D = 1 << (Q - 6);
#pragma unroll
        for (int k = 0; k < R; k++)
            if ((k & D) == 0) h_butterfly(r[k], r[k + D]);
    }
}

template <int Q, int R, bool NTL, bool NTS, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_h_wave(amp_t *__restrict__ amp, uint64_t ntiles, unsigned glog, unsigned slog)
{
    // tile = 64*R amplitudes, one per wave per iteration; slog: stream-interleaved block order as in k_h_pair
    const unsigned lane = threadIdx.x & 63u;
    uint64_t blk = blockIdx.x;
    if (slog) blk = ((uint64_t)(blockIdx.x & ((1u << slog) - 1u)) << (glog - slog)) | (blockIdx.x >> slog);      // (= stream_tile(), spelled out: see there)
    const uint64_t wave = (blk * BLOCK + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * BLOCK) >> 6;
    for (uint64_t t = wave; t < ntiles; t += nwaves) {
        amp_t *base = amp + t * (64 * R) + lane;
        amp_t r[R];
#pragma unroll
        for (int k = 0; k < R; k++) r[k] = ld<NTL>(base + k * 64);
        h_wave_tile<Q, R>(r, lane);
#pragma unroll
        for (int k = 0; k < R; k++) st<NTS>(base + k * 64, r[k]);
    }
}

// ---------------------------------------------------------------------------
// K2  controlled phase: multiply by (c + i s) every amplitude whose index has
// all NB mask bits set (b0 < b1).  Only that 1/2^NB of the vector is touched.
// ---------------------------------------------------------------------------
template <int NB, int APT, bool NT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_phase(amp_t *__restrict__ amp, unsigned b0, unsigned b1,
                                                   double c, double s, uint64_t count, unsigned glog, unsigned slog)
{
    const uint64_t step = (uint64_t)gridDim.x * (BLOCK * APT);
    uint64_t tile0 = blockIdx.x;              // stream-interleaved tile order as in k_h_pair
    if (slog) tile0 = ((uint64_t)(blockIdx.x & ((1u << slog) - 1u)) << (glog - slog)) | (blockIdx.x >> slog);      // (= stream_tile(), spelled out: see there)
    for (uint64_t base = tile0 * (BLOCK * APT); base < count; base += step) {
        amp_t v[APT];
        uint64_t idx[APT];
#pragma unroll
        for (int k = 0; k < APT; k++) {
            const uint64_t p = base + (uint64_t)k * BLOCK + threadIdx.x;
            uint64_t i = p;
            if (NB >= 1) i = insert_zero(i, b0) | ((uint64_t)1 << b0);
            if (NB >= 2) i = insert_zero(i, b1) | ((uint64_t)1 << b1);
            idx[k] = i;
            if (p < count) v[k] = ld<NT>(amp + i);
        }
#pragma unroll
        for (int k = 0; k < APT; k++) {
            const uint64_t p = base + (uint64_t)k * BLOCK + threadIdx.x;
            if (p < count) {
                amp_t o;
                o.x = ((c * v[k].x) - (s * v[k].y)) + 0.0;      // Q:409
                o.y = ((c * v[k].y) + (s * v[k].x)) + 0.0;      // Q:412
                st<NT>(amp + idx[k], o);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// K2b  controlled phase whose mask has a bit below 3, i.e. inside a 128-B line (8 amplitudes).  k_phase above gives
// every lane one TOUCHED amplitude, so for such masks a wave instruction reads 16 B out of every 32 or 64: twice to four
// times the requests for the same lines.  Here a lane owns one amplitude of every touched LINE (the mask bits >= 3
// are squeezed out of the numbering, the bits < 3 stay free): whole-line coalesced loads, the rotation only where the
// low mask bits are set, and stores of the rotated lanes only -- except at 16- or 32-B granularity (mask bit 0 or 1),
// where the whole line is stored back (untouched amplitudes with the bits they had): masked 32-B stores measured
// 4.0 ms against 2.6 ms at n = 30.
// NH = number of mask bits >= 3 (0, 1 or 2): h0 < h1.
// ---------------------------------------------------------------------------
template <int NH, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_phase_lines(amp_t *__restrict__ amp, unsigned h0, unsigned h1, unsigned lowmask, int store_all,
                                                         double c, double s, uint64_t count, unsigned glog, unsigned slog)
{
    const uint64_t step = (uint64_t)gridDim.x * BLOCK;
    uint64_t tile0 = blockIdx.x;
    if (slog) tile0 = ((uint64_t)(blockIdx.x & ((1u << slog) - 1u)) << (glog - slog)) | (blockIdx.x >> slog);      // (= stream_tile(), spelled out: see there)
    for (uint64_t p = tile0 * BLOCK + threadIdx.x; p < count; p += step) {
        uint64_t i = p;
        if (NH >= 1) i = insert_zero(i, h0) | ((uint64_t)1 << h0);
        if (NH >= 2) i = insert_zero(i, h1) | ((uint64_t)1 << h1);
        const amp_t v = __builtin_nontemporal_load(amp + i);
        const bool hit = ((unsigned)i & lowmask) == lowmask;
        amp_t o = v;
        if (hit) {
            o.x = ((c * v.x) - (s * v.y)) + 0.0;      // Q:409
            o.y = ((c * v.y) + (s * v.x)) + 0.0;      // Q:412
        }
        if (hit || store_all) __builtin_nontemporal_store(o, amp + i);
    }
}

// ---------------------------------------------------------------------------
// K3  controlled modular multiply on the low M bits (Q:595-660).  Pure data
// movement: destination g (< C) of every 2^M-block with the control bit set
// receives the sum, in ascending source order, of the amplitudes at the
// sources f < C with (A*f) mod C == g.  With d = gcd(A, C) those are
//     f = f0 + t*(C/d),  t = 0..d-1,  f0 = ((g/d) * inv) mod (C/d),  d | g
// (inv = (A/d)^-1 mod C/d, computed on the host); for the usual coprime case
// d = 1 and the gate is a permutation.  A tile of 2^logT >= 2^M amplitudes is
// staged in LDS so the update is in place with coalesced global traffic; the
// amplitudes whose control bit is 0 are never touched (camodc_tile).
// ---------------------------------------------------------------------------

struct CamodcParams {
    unsigned M, logT;
    int      ctl;        // local bit index, or -1: control lives in the rank id and is 1
    unsigned C, d, Cd, inv;
    uint64_t ntiles;     // tiles to process (tiles hold control-set amplitudes only when ctl >= M)
    unsigned skip, ntl;  // k_camodc: do not read the lines above row C; store completely rewritten lines nontemporally
};

// base of tile tt.  A tile is 2^logT amplitudes that all have the control bit SET: a control at or
// above the M register is squeezed out of the tile numbering (whether it lies above the tile or inside it), so the
// control-clear half of the vector is never read.  Runs stay >= 2^M amplitudes (the control is never below M here).
__device__ __forceinline__ amp_t *camodc_tile(amp_t *amp, const CamodcParams &P, uint64_t tt)
{
    if (P.ctl >= (int)P.logT) {
        const unsigned b = (unsigned)P.ctl - P.logT;
        return amp + ((insert_zero(tt, b) | ((uint64_t)1 << b)) << P.logT);
    }
    if (P.ctl >= (int)P.M) return amp + (tt << (P.logT + 1));
    return amp + (tt << P.logT);
}
// offset of tile element e from camodc_tile(): with the control inside the tile, e with a 1 inserted at the control bit
__device__ __forceinline__ unsigned camodc_elem(bool squeeze, unsigned ctl, unsigned e)
{
    if (!squeeze) return e;
    const unsigned low = (1u << ctl) - 1u;
    return ((e & ~low) << 1) | (1u << ctl) | (e & low);
}

// (A variant that stored every amplitude of the tile back as whole nontemporal lines -- 32 B per amplitude instead of 16 + 16 * C / 2^M,
// no partial-line writes -- measured 2.9-3.4 against 2.8-2.9 ms in round 3 and was removed in round 5.)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_camodc(amp_t *__restrict__ amp, CamodcParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char qcx_lds_raw[];
    amp_t *tile = reinterpret_cast<amp_t *>(qcx_lds_raw);
    const unsigned T = 1u << P.logT, blkmask = (1u << P.M) - 1u;
    const bool squeeze = P.ctl >= (int)P.M && P.ctl < (int)P.logT;
    // the permutation case (gcd(A, C) = 1): the source row of every destination row, tabulated once per workgroup -- one
    // 32-bit modulo per residue instead of two divisions and a modulo per amplitude (round 4: 2.85 -> 2.4 ms at n = 30 together
    // with the skipped lines)
    unsigned short *lut = reinterpret_cast<unsigned short *>(tile + T);
    const bool perm = P.d == 1u && P.M <= 12u;
    if (perm) for (unsigned f = threadIdx.x; f <= blkmask; f += BLOCK) lut[f] = (unsigned short)(f < P.C ? (f * P.inv) % P.C : f);
    for (uint64_t tt = blockIdx.x; tt < P.ntiles; tt += gridDim.x) {
        amp_t *g = camodc_tile(amp, P, tt);
        // (fill through registers with the DEFAULT cache policy, measured at n = 30: 2.9 ms per gate; an LDS-DMA fill 3.0-3.2 ms;
        // nontemporal loads 4.1-4.5 ms -- the moved elements are rewritten as PARTIAL lines a moment later and those
        // writes must still find their lines in L2)
        // Rows f >= C of a 2^M block are neither sources nor destinations (Q:631-634): the 128-B lines that hold nothing
        // else are not even read (round 4; C = 21, M = 5: one line in four).  lineC = C rounded up to whole lines.
        const unsigned lineC = P.skip ? ((P.C + 7u) & ~7u) : (1u << P.M);
        for (unsigned e = threadIdx.x; e < T; e += BLOCK)
            if ((e & blkmask) < lineC) tile[e] = g[camodc_elem(squeeze, (unsigned)P.ctl, e)];
        __syncthreads();
        const unsigned fullC = P.ntl ? (P.C & ~7u) : 0u;                 // rows below this sit in lines that are rewritten completely
        for (unsigned e = threadIdx.x; e < T; e += BLOCK) {
            const unsigned f = e & blkmask;
            bool on = true;
            if (P.ctl >= 0 && P.ctl < (int)P.M) on = (e >> P.ctl) & 1u;
            if (!on || f >= P.C) continue;                     // identity rows (Q:611-613, Q:631-634)
            amp_t acc; acc.x = 0.0; acc.y = 0.0;
            if (perm) { const amp_t sv = tile[(e - f) + lut[f]]; acc.x += sv.x; acc.y += sv.y; }
            else if (f % P.d == 0) {
                unsigned src = ((f / P.d) * P.inv) % P.Cd;            // < C^2 <= 2^32: 32-bit arithmetic is exact (host checks)
                const amp_t *blk = tile + (e - f);
                for (unsigned t = 0; t < P.d; t++, src += P.Cd) { acc.x += blk[src].x; acc.y += blk[src].y; }
            }
            // whole rewritten lines leave as nontemporal stores, the partly rewritten last line of a block through L2
            if (f < fullC && P.ctl >= (int)P.M) __builtin_nontemporal_store(acc, g + camodc_elem(squeeze, (unsigned)P.ctl, e));
            else g[camodc_elem(squeeze, (unsigned)P.ctl, e)] = acc;
        }
        __syncthreads();
    }
}

// (Round 5 tried the permutation case WITHOUT the LDS tile for blocks that fit a wave (M <= 6): lane l loads its amplitude, the
// destination lanes fetch theirs by shuffle, four tiles of 64 amplitudes per wave in flight, no barrier.  Slower: 2.52 ms per gate
// at n = 30 against 2.33 for k_camodc (2.42 when it writes whole lines with nontemporal traffic); the counters of k_camodc --
// 71 % of wave cycles waiting, traffic exactly the touched lines -- and this experiment say the same thing: the gate is bound by
// the memory side's handling of 3-lines-in-4 read-modify-write traffic, not by the workgroups' load -> barrier -> store chains.
// profiles/r05g_camodc_*.json, profiles/r05_camodc_wave_experiment.txt.  Removed again.)
// generic table form (C > 2^M, or 32-bit wrap in A*f): CSR of sources per
// destination low-bits value, built on the host exactly as Q:619-647 maps them.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_camodc_table(amp_t *__restrict__ amp, CamodcParams P,
                                                          const uint32_t *__restrict__ off,
                                                          const uint32_t *__restrict__ srcs)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char qcx_lds_raw[];
    amp_t *tile = reinterpret_cast<amp_t *>(qcx_lds_raw);
    const unsigned T = 1u << P.logT, blkmask = (1u << P.M) - 1u;
    const bool squeeze = P.ctl >= (int)P.M && P.ctl < (int)P.logT;
    for (uint64_t tt = blockIdx.x; tt < P.ntiles; tt += gridDim.x) {
        amp_t *g = camodc_tile(amp, P, tt);
        for (unsigned e = threadIdx.x; e < T; e += BLOCK) tile[e] = g[camodc_elem(squeeze, (unsigned)P.ctl, e)];
        __syncthreads();
        for (unsigned e = threadIdx.x; e < T; e += BLOCK) {
            const unsigned f = e & blkmask;
            // (a control inside the M register is encoded in the table: the host passes ctl = -1 then)
            const amp_t *blk = tile + (e - f);
            amp_t acc; acc.x = 0.0; acc.y = 0.0;
            for (uint32_t k = off[f]; k < off[f + 1]; k++) { acc.x += blk[srcs[k]].x; acc.y += blk[srcs[k]].y; }
            g[camodc_elem(squeeze, (unsigned)P.ctl, e)] = acc;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// K0 helpers
// ---------------------------------------------------------------------------
__global__ void k_set_one(amp_t *amp, uint64_t index)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) { amp_t v; v.x = 1.0; v.y = 0.0; amp[index] = v; }
}

// synthetic input: counter-based pseudo-random amplitudes, component k of the whole vector is
//   ((splitmix64(seed + k) >> 11) * 2^-53 - 0.5) * scale      (k = 2*index + {0: re, 1: im})
// every operation exact or singly rounded, so the CPU twin in oracle/ gives the same bits and a
// window of a 16-GiB state can be checked without ever holding it on the host.
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

__global__ __launch_bounds__(256) void k_fill_random(amp_t *__restrict__ amp, uint64_t count, uint64_t first_global,
                                                     uint64_t seed, double scale)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256) {
        const uint64_t k = 2 * (first_global + i);
        amp_t v;
        v.x = ((double)(splitmix64(seed + k) >> 11) * 0x1p-53 - 0.5) * scale;
        v.y = ((double)(splitmix64(seed + k + 1) >> 11) * 0x1p-53 - 0.5) * scale;
        amp[i] = v;
    }
}

// ---------------------------------------------------------------------------
// K0c  canonical zeros.  The reference's mat-vec rewrites EVERY amplitude at every gate as 0 + 1.0 * x (+ ...) (Q:393-413),
// which turns a -0 component into +0 even where the gate is the identity.  The gate kernels only touch the amplitudes a
// gate acts on, so they rely on an invariant instead: the state holds no -0 whenever a gate runs.  Reset, collapse, the
// synthetic fill and every gate kernel keep it (each result ends in "+ 0.0"); a state WRITTEN by the caller
// (qcx_state_write / qcx_state_load) may break it, and is passed through this kernel once before the next gate.
// Reads everything, stores only the amplitudes that change.
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// K9  STRICT gates for states that hold non-finite (or overflow-prone) amplitudes (round 5).  The gate kernels above give the
// reference's bits for every FINITE state while skipping what the reference's mat-vec spends on nothing: the products with
// the matrix entries' zero imaginary parts, and the rows whose entry is 1.  With an Inf or NaN in the state those are not
// nothing: 0 * Inf = NaN poisons the other component of the SAME amplitude, through an identity row too (Q:409-412 runs
// over every stored triplet).  A register that was handed such values (qcx_state_write / _load; the host sets
// qcx_register::nonfinite from a scan of what was written) runs every gate through these kernels instead -- one plain pass
// per gate over ALL amplitudes with the mat-vec's own four products and sums per triplet (Q:396-413 applied to
// the triplets each gate stores, Q:456-481 / Q:529-562 / Q:612-657) -- until a reset, a fill or a measurement replaces the state.  z and one arrive as
// kernel arguments so that no compiler ever folds a product with them.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_strict_h(amp_t *__restrict__ amp, unsigned n, unsigned q, double s, double z)
{
    const uint64_t half = (uint64_t)1 << (n - 1), bitq = (uint64_t)1 << q, low = bitq - 1;
    for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < half; p += (uint64_t)gridDim.x * 256u) {
        const uint64_t i0 = ((p & ~low) << 1) | (p & low), i1 = i0 | bitq;
        const amp_t a = amp[i0], b = amp[i1];
        const amp_t lo = q_row(q_mul(s, z, a), q_mul(s, z, b));    // row i0: columns i0, i1
        const amp_t hi = q_row(q_mul(s, z, a), q_mul(-s, z, b));   // row i1
        amp[i0] = lo; amp[i1] = hi;
    }
}

__global__ __launch_bounds__(256) void k_strict_phase(amp_t *__restrict__ amp, uint64_t count, uint64_t both, double er, double ei, double one, double z)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256u) {
        const amp_t v = amp[i];
        amp[i] = (i & both) == both ? q_row(q_mul(er, ei, v)) : q_row(q_mul(one, z, v));
    }
}

// one workgroup per 2^M-block (M <= 12: the block and the destination of every row sit in LDS); destination g sums its sources
// in ascending row order, every row of the block is written (the identity rows too: their entry 1 is a triplet like any other)
__global__ __launch_bounds__(256) void k_strict_camodc(amp_t *__restrict__ amp, unsigned n, unsigned M, unsigned C, unsigned A, int ctl, double one, double z)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char qcx_lds_raw[];
    amp_t *blk = reinterpret_cast<amp_t *>(qcx_lds_raw);
    const unsigned B = 1u << M;
    unsigned short *dst_on = reinterpret_cast<unsigned short *>(blk + B);         // destination of row f when its control reads 1
    for (unsigned f = threadIdx.x; f < B; f += 256u) dst_on[f] = (unsigned short)(f < C ? ((unsigned)(A * f) % C) & (B - 1u) : f);   // Q:645-647
    const uint64_t nblk = (uint64_t)1 << (n - M);
    for (uint64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        amp_t *g = amp + (b << M);
        __syncthreads();
        for (unsigned f = threadIdx.x; f < B; f += 256u) blk[f] = g[f];
        __syncthreads();
        const int on = (ctl >= (int)M) ? (int)(((b << M) >> ctl) & 1u) : -1;      // -1: the control is a bit of the row
        for (unsigned d = threadIdx.x; d < B; d += 256u) {
            amp_t acc = q_row();                                   // (a row of as many triplets as sources map to d)
            for (unsigned f = 0; f < B; f++) {
                const bool cbit = on >= 0 ? on != 0 : ((f >> ctl) & 1u) != 0;
                const unsigned to = cbit ? dst_on[f] : f;
                if (to == d) { const q_mul p(one, z, blk[f]); acc.x += p.re(); acc.y += p.im(); }
            }
            g[d] = acc;
        }
    }
}

// does [amp, amp + count) hold a component that is not finite, or so large (>= 2^500) that a circuit could overflow from it?
__global__ __launch_bounds__(256) void k_scan_nonfinite(const amp_t *__restrict__ amp, uint64_t count, unsigned *flag)
{
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256u) {
        const amp_t v = amp[i];
        bad |= !(fabs(v.x) < 0x1p500) || !(fabs(v.y) < 0x1p500);
    }
    if (__ballot(bad) && (threadIdx.x & 63u) == 0u) atomicOr(flag, 1u);
}

__global__ __launch_bounds__(256) void k_canon_zeros(amp_t *__restrict__ amp, uint64_t count)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256) {
        amp_t v = __builtin_nontemporal_load(amp + i);
        const bool neg0 = (uint64_t)__double_as_longlong(v.x) == 0x8000000000000000ULL || (uint64_t)__double_as_longlong(v.y) == 0x8000000000000000ULL;
        if (neg0) { v.x += 0.0; v.y += 0.0; amp[i] = v; }
    }
}

// ---------------------------------------------------------------------------
// K5  total probability.  Deterministic two-stage tree (fixed grid), not the
// reference's sequential order (T:28-37) -- a check value, compared with a
// tolerance.
// ---------------------------------------------------------------------------
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_norm_partial(const amp_t *__restrict__ amp, uint64_t count, double *partial)
{
    __shared__ double red[BLOCK / 64];
    double acc = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < count; i += (uint64_t)gridDim.x * BLOCK) {
        const amp_t v = amp[i];
        acc += v.x * v.x + v.y * v.y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < BLOCK / 64; w++) t += red[w];
        partial[blockIdx.x] = t;
    }
}

__global__ void k_norm_final(const double *partial, unsigned nparts, double *out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double t = 0.0;
        for (unsigned i = 0; i < nparts; i++) t += partial[i];
        *out = t;
    }
}

// ---------------------------------------------------------------------------
// K4  measurement scan, exact form: the reference's strictly sequential
// cumulative sum (Q:283-292) carried by ONE wave.  Lanes fetch 64 amplitudes
// at a time (coalesced) and the 64 additions are chained in index order; lane
// k ends each round holding the running sum through element k, so the first
// lane with cum >= r is the reference's answer bit for bit.
// ---------------------------------------------------------------------------
struct MeasureOut {
    int      found;
    uint64_t index;
    double   cum;
    unsigned stats[2];          // K4c: [records looked at closely, records] of the scan (qcx_measure_last_stats): one copy back with the result
};

__device__ __forceinline__ double readlane_f64(double v, int lane)
{
    union { double d; int i[2]; } u; u.d = v;
    u.i[0] = __builtin_amdgcn_readlane(u.i[0], lane);
    u.i[1] = __builtin_amdgcn_readlane(u.i[1], lane);
    return u.d;
}

__global__ __launch_bounds__(64) void k_measure_scan(const amp_t *__restrict__ amp, uint64_t count,
                                                     double cum_in, double r, MeasureOut *out)
{
    const unsigned lane = threadIdx.x;
    double cum = cum_in;
    amp_t nxt; nxt.x = 0.0; nxt.y = 0.0;
    if (lane < count) nxt = amp[lane];
    for (uint64_t base = 0; base < count; base += 64) {
        const amp_t v = nxt;
        const uint64_t ni = base + 64 + lane;
        nxt.x = 0.0; nxt.y = 0.0;
        if (ni < count) nxt = amp[ni];                       // prefetch the next round
        const double p = v.x * v.x + v.y * v.y;              // gsl_complex_abs2 (Q:286); 0 past the end
        double run = cum;
#pragma unroll
        for (int j = 0; j < 64; j++) {
            const double pj = readlane_f64(p, j);
            run = run + ((int)lane >= j ? pj : 0.0);         // + 0.0 leaves a non-negative sum unchanged
        }
        const bool hit = (base + lane < count) && (run >= r);
        const unsigned long long m = __ballot(hit);
        if (m) {
            const int first = __builtin_ctzll(m);
            if ((int)lane == first) { out->found = 1; out->index = base + lane; out->cum = run; }
            return;
        }
        cum = readlane_f64(run, 63);
    }
    if (lane == 0) { out->found = 0; out->index = 0; out->cum = cum; }
}

// ---------------------------------------------------------------------------
// K4  exact AND parallel measurement scan: the arithmetic fact K4c below rests on.
//
// The reference's cumulative sum cum_i = fl(cum_{i-1} + p_i) is order dependent, so a parallel
// prefix sum does not give the same decisions.  But while the running sum stays inside one binade
// [2^e, 2^(e+1)) it is an integer K (53 bits) times the fixed ulp u = 2^(e-52), and adding p >= 0
// rounds to   K + floor(p/u) + [frac(p/u) > 1/2]        (a tie, frac == 1/2, rounds to even).
// So for a block of amplitudes with no tie and no element >= 2^e, the sequential sum over the block is
// exactly K + S with S = sum_i (floor(p_i/u) + [frac > 1/2]) -- an ORDINARY integer sum -- provided
// K + S < 2^53 (no binade crossing).  A block whose binade guess holds costs a few integer operations; any
// other block (binade crossing, wrong guess, tie, start of the sum, the block in which cum reaches r) is redone
// with a strictly sequential scan.  The result is the reference's index, bit for bit, for every input; only the
// speed depends on the data.  (Round 3's two-read form of this, K4b -- tree block sums for the guesses, then the
// increments, then a one-wave chain over the records: 7 ms at n = 30 -- was removed in round 5; K4c reads once.)
// ---------------------------------------------------------------------------
// amplitudes per record = 2^blog, a launch parameter (8..11; host: meas_block_log): small registers want small records
enum : uint32_t { MEAS_ALLZERO = 1u << 16, MEAS_TIE = 1u << 17, MEAS_BIG = 1u << 18, MEAS_EUNK = 1u << 19 };
// MEAS_RHIT (round 5): the APPROXIMATE running sum reaches r inside this record (with a margin) -- a hint for k_meas_fast's
// list of records to look at closely; it decides nothing
enum : uint32_t { MEAS_RHIT = 1u << 20 };

struct MeasBlock {
    uint64_t S;        // integer increment of the block in units of the assumed ulp (saturated)
    uint32_t meta;     // low 11 bits: assumed biased exponent of the running sum at block start; flags above
    uint32_t pad;
};

__device__ __forceinline__ double prob_of(amp_t v) { return v.x * v.x + v.y * v.y; }    // gsl_complex_abs2

// ---------------------------------------------------------------------------
// K4c  measurement scan, exact and parallel, in ONE read of the state (round 4).
//
//   1. k_meas_onepass   a workgroup of four waves takes four consecutive RECORDS of 2^RLOG amplitudes (one per wave, kept
//                       as |amp|^2 in registers), publishes the (tree) sum of the four, obtains the approximate sum of
//                       everything before it by a DECOUPLED LOOK-BACK, and every wave computes the integer increment S of
//                       its record under the binade that prefix falls in -- one pass over HBM.  Workgroup ids are handed
//                       out by an atomic ticket, so a workgroup only ever waits for workgroups that are already running.
//                       The XCDs' L2s are not coherent, so every poll is a round trip to the memory side, and ~1300
//                       workgroups run at once: polling their slots one by one costs more traffic than it hides (measured:
//                       +0.45 ms per 16 GiB with 64 slots per poll, +2.3 ms with 512).  The look-back therefore has two
//                       levels: the last member of every group of 64 workgroups publishes the group's sum as soon as it has seen
//                       the other 63, and a later workgroup reads (a) the slots of the earlier members of its own group and
//                       (b) ONE entry per earlier group -- its sum, or the running total through it.
//                       The look-back only feeds the GUESS: the order of the approximate additions may differ from run to
//                       run; the walk below validates every guess against the exact running sum, so the measured index
//                       never depends on it;
//   2. k_meas_groups    sums of 64, 64^2, ... consecutive records (a few tiny launches);
//   3. k_meas_fast      (round 5, further down) the EVENTS of the scan from a list of candidate records the groups launch wrote:
//                       8 waves, stretch sums and record data prepared in parallel, ~1 us of serial work per event;
//   4. k_meas_walk      the fallback behind it, and the whole of step 3 in round 4:
//                       one wave descends that tree with the EXACT running sum: 64 entries per step, whole groups at a
//                       time while they are plain (integer additions inside one binade are associative); only a record with
//                       a tie, an oversized element, a wrong guess, a binade crossing or the crossing of r is redone: as one
//                       integer addition per 1024 amplitudes where that holds, per 64 below that, and the strictly
//                       sequential chain only for the 64 amplitudes in which something happens.
// ---------------------------------------------------------------------------
typedef unsigned long long meas_slot_t;      // bits of a double; all ones = not published yet

struct MeasLookback {
    meas_slot_t *agg, *incl;                 // per workgroup: its sum / the running total through it
    meas_slot_t *gsum, *gincl;               // per group of 64 workgroups: the group's sum (published by its last member) / the running total through it
    unsigned    *ticket;
};

__device__ __forceinline__ uint64_t meas_inc(uint64_t b, int e, uint32_t &flags)    // b = bits of p > 0; increment of the running sum in ulps of binade e
{
    // branch-free (the callers unroll this 32 times): p/u = mp * 2^-sh, rounded to nearest; a tie (fraction exactly 1/2) is
    // flagged, as is an element at or above the binade (sh <= 0).  sh = 53: quotient 0, remainder mp against half = 2^52;
    // sh >= 54: half > mp, the increment is 0 (the shift is clamped to 63 for the far-away exponents).
    const int ex = (int)((b >> 52) & 0x7ff);
    const uint64_t mp = (b & 0xfffffffffffffULL) | (ex ? (uint64_t)1 << 52 : 0);       // subnormal: no implicit bit
    const int sh = e - (ex ? ex : 1);
    const bool big = sh <= 0;
    const unsigned shc = (unsigned)(sh < 1 ? 1 : (sh > 63 ? 63 : sh));
    const uint64_t rem = mp & (((uint64_t)1 << shc) - 1), half = (uint64_t)1 << (shc - 1);
    const uint64_t inc = (mp >> shc) + (rem > half ? 1u : 0u);
    flags |= big ? (uint32_t)MEAS_BIG : (rem == half ? (uint32_t)MEAS_TIE : 0u);
    return big ? (uint64_t)1 << 54 : inc;
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return readlane_f64(v, 0);
}
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int lane)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), lane) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(v & 0xffffffffu), lane);
}
__device__ __forceinline__ meas_slot_t meas_poll(const meas_slot_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void meas_post(meas_slot_t *p, double v) { __hip_atomic_store(p, (meas_slot_t)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one look-back window: lane l holds the slot at distance l (vi = a running total, or all ones; va = a plain sum, or all
// ones; lanes at or beyond `lanes` hold nothing).  1: a running total was found and `run` is complete; 0: all `lanes`
// sums consumed, go on further back; -1: a slot before the first running total is still unpublished
__device__ __forceinline__ int meas_window(unsigned lane, unsigned lanes, meas_slot_t vi, meas_slot_t va, double &run)
{
    const bool in = lane < lanes;
    const bool has_i = in && vi != ~0ULL, has_a = has_i || (in && va != ~0ULL);
    const unsigned long long mi = __ballot(has_i), ma = __ballot(has_a);
    const unsigned first = mi ? (unsigned)__builtin_ctzll(mi) : lanes;          // slots before it must have published their sums
    const unsigned long long need = first >= 64 ? ~0ULL : (((unsigned long long)1 << first) - 1);
    if ((ma & need) != need) return -1;
    double c = 0.0;
    if (lane < first) c = __longlong_as_double((long long)va);
    else if (lane == first && mi) c = __longlong_as_double((long long)vi);
    run += wave_sum_f64(c);
    return mi ? 1 : 0;
}

template <int RLOG>
__global__ __launch_bounds__(256) void k_meas_onepass(const amp_t *__restrict__ amp, uint64_t count, double cum_in,
                                                       MeasLookback LB, MeasBlock *out, unsigned spin_limit, unsigned dbg, double r)
{
    constexpr unsigned PER = (1u << RLOG) / 64u;            // amplitudes per lane: 4 .. 32
    __shared__ unsigned s_blk;
    __shared__ double red[4];
    __shared__ uint64_t s_pref;
    if (threadIdx.x == 0) s_blk = atomicAdd(LB.ticket, 1u);
    __syncthreads();
    const unsigned blk = s_blk, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t rec = (uint64_t)blk * 4u + wave;
    const uint64_t base = rec << RLOG;
    double p[PER];
    // loads in batches of 8 (8 x 16 B in flight per lane); the record's probabilities stay in registers
    constexpr unsigned BATCH = PER < 8u ? PER : 8u;
    if (((uint64_t)(blk + 1u) << (RLOG + 2)) <= count) {            // (all workgroups but the last: no per-load bounds test)
#pragma unroll
        for (unsigned kb = 0; kb < PER; kb += BATCH) {
            amp_t v[BATCH];
#pragma unroll
            for (unsigned g = 0; g < BATCH; g++) v[g] = __builtin_nontemporal_load(amp + base + (uint64_t)(kb + g) * 64u + lane);
#pragma unroll
            for (unsigned g = 0; g < BATCH; g++) p[kb + g] = prob_of(v[g]);
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
#pragma unroll
        for (unsigned k = 0; k < PER; k++) {            // (unrolled too: a run-time index would put p[] into scratch memory)
            const uint64_t i = base + (uint64_t)k * 64u + lane;
            double pk = 0.0;
            if (i < count) pk = prob_of(amp[i]);
            p[k] = pk;
        }
    }
    double acc = 0.0;
#pragma unroll
    for (unsigned k = 0; k < PER; k++) acc += p[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x < 64) {
        double t = (red[0] + red[1]) + (red[2] + red[3]);
        if (!(t < __builtin_inf())) t = __builtin_inf();          // NaN / Inf input: every later guess is "unknown" (exact path)
        const unsigned g = blk >> 6, q = blk & 63u;
        if (lane == 0) meas_post(&LB.agg[blk], t);
        double run = 0.0;
        int state = (dbg & 1u) ? 1 : 0;                            // dbg bit 0 (diagnostics): no look-back, every guess from cum_in alone
        if (state) run = cum_in;
        unsigned spins = 0;
        // (a) the earlier members of this workgroup's own group, nearest first.  The LAST member of a group (q = 63) waits for
        // all 63 sums whether or not a running total turns up among them: it publishes the group's sum (no atomics: float
        // atomic adds from every workgroup plus a release-ordered count cost 6 ms per 16 GiB when tried)
        while (state == 0 && q > 0) {
            meas_slot_t vi = ~0ULL, va = ~0ULL;
            if (lane < q) { vi = meas_poll(&LB.incl[blk - 1u - lane]); if (vi == ~0ULL || q == 63u) va = meas_poll(&LB.agg[blk - 1u - lane]); }
            bool ready = true;
            if (q == 63u) {
                ready = __ballot(lane < q && va == ~0ULL) == 0ULL;
                if (ready) {
                    double gs = wave_sum_f64(lane < q ? __longlong_as_double((long long)va) : 0.0) + t;
                    if (!(gs < __builtin_inf())) gs = __builtin_inf();
                    if (lane == 0) meas_post(&LB.gsum[g], gs);
                }
            }
            const int w = ready ? meas_window(lane, q, vi, va, run) : -1;
            if (w >= 0) { state = w; break; }
            if (++spins > spin_limit) { state = -1; break; }
            __builtin_amdgcn_s_sleep(32);
        }
        // (b) whole groups before it, nearest first; "group -1" holds cum_in
        int64_t gj = (int64_t)g - 1;
        while (state == 0) {
            const int64_t gi = gj - (int64_t)lane;
            meas_slot_t vi = ~0ULL, va = ~0ULL;
            unsigned lanes = 64;
            if (gj < 63) lanes = (unsigned)(gj + 2);               // groups gj .. 0, then the virtual one
            if (gi == -1) vi = (meas_slot_t)__double_as_longlong(cum_in);
            else if (gi >= 0) { vi = meas_poll(&LB.gincl[gi]); if (vi == ~0ULL) va = meas_poll(&LB.gsum[gi]); }
            const int w = meas_window(lane, lanes, vi, va, run);
            if (w > 0) { state = 1; break; }
            if (w == 0) { gj -= 64; continue; }
            if (++spins > spin_limit) { state = -1; break; }       // (never seen; a bound, so that nothing can hang)
            __builtin_amdgcn_s_sleep(32);
        }
        if (state < 0) run = __builtin_inf();
        if (lane == 0) {
            double through = run + t;
            if (!(through < __builtin_inf())) through = __builtin_inf();
            meas_post(&LB.incl[blk], through);
            if (q == 63u) meas_post(&LB.gincl[g], through);
            s_pref = (uint64_t)__double_as_longlong(run);
        }
    }
    __syncthreads();
    double pref = __longlong_as_double((long long)s_pref);
    for (unsigned w = 0; w < wave; w++) pref += red[w];           // the waves before this one in the workgroup
    const int e = (int)(((uint64_t)__double_as_longlong(pref) >> 52) & 0x7ff);
    uint64_t S = 0;
    uint32_t flags = (e == 0 || e == 0x7ff) ? (uint32_t)MEAS_EUNK : 0u;
    if (pref <= r * (1.0 + 1e-9) && pref + red[wave] >= r * (1.0 - 1e-9)) flags |= (uint32_t)MEAS_RHIT;
    bool nonzero = false;
    const uint64_t SAT = (uint64_t)1 << 54;
#pragma unroll
    for (unsigned k = 0; k < PER; k++) {
        const uint64_t b = (uint64_t)__double_as_longlong(p[k]);
        uint32_t f1 = 0;
        const uint64_t inc = meas_inc(b, e, f1);
        nonzero |= b != 0;
        S += b ? inc : 0;
        flags |= b ? f1 : 0u;
        if (S > SAT) S = SAT;
    }
    const unsigned long long any_nz = __ballot(nonzero);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        S += (uint64_t)__shfl_down((unsigned long long)S, o, 64);
        flags |= (uint32_t)__shfl_down((int)flags, o, 64);
    }
    if (lane == 0) {
        if (S > SAT) S = SAT;
        MeasBlock mb; mb.S = S; mb.meta = (uint32_t)e | (flags & 0x7fff0000u) | (any_nz ? 0u : (uint32_t)MEAS_ALLZERO); mb.pad = 0;
        out[rec] = mb;
    }
}

// one level up: record g = 64 consecutive records of the level below (one wave each).  A group is PLAIN when all its
// non-zero members are unflagged and were computed under the same binade; anything else sets MEAS_EUNK = "descend".
// cands (the launch over the records themselves only): the records k_meas_fast has to look at closely -- flagged ones, and both
// sides of every change of the binade guess (a crossing lies in one of the two)
#define QCX_MEAS_CAND_CAP 192u
struct MeasCands { unsigned count, pad; unsigned ticket[4]; unsigned list[QCX_MEAS_CAND_CAP]; };    // ticket: the look-back's workgroup counter (a fixed address whatever the scan's size)

__global__ __launch_bounds__(64) void k_meas_groups(const MeasBlock *__restrict__ in, unsigned nin, MeasBlock *__restrict__ outg, MeasCands *cands,
                                                    meas_slot_t *look, unsigned nslots)
{
    const unsigned lane = threadIdx.x, i = blockIdx.x * 64u + lane;
    // (the launch over the records also puts the look-back's slots back to "not published" for the next scan -- k_meas_onepass is
    //  through with them: one memset launch less per measurement.  The slots only feed guesses: a stale one costs time, never a result)
    if (look) {
        const unsigned per = (nslots + gridDim.x - 1u) / gridDim.x;
        for (unsigned k = lane; k < per; k += 64u) { const unsigned idx = blockIdx.x * per + k; if (idx < nslots) look[idx] = ~0ULL; }
    }
    MeasBlock m; m.S = 0; m.meta = MEAS_ALLZERO; m.pad = 0;
    if (i < nin) m = in[i];
    const bool zero = (m.meta & MEAS_ALLZERO) != 0;
    if (cands) {
        const int e_me = (int)(m.meta & 0x7ffu);
        int e_next = __shfl_down(e_me, 1, 64), e_prev = __shfl_up(e_me, 1, 64);
        if (lane == 63u && i + 1u < nin) e_next = (int)(in[i + 1u].meta & 0x7ffu);
        if (lane == 0u) e_prev = i > 0u ? (int)(in[i - 1u].meta & 0x7ffu) : e_me;
        if (i + 1u >= nin) e_next = e_me;
        const bool c = i < nin && ((!zero && (m.meta & (MEAS_TIE | MEAS_BIG | MEAS_EUNK | MEAS_RHIT))) || e_next != e_me || e_prev != e_me);
        const unsigned long long cm = __ballot(c);
        if (cm) {
            unsigned base = 0;
            if (lane == 0u) base = atomicAdd(&cands->count, (unsigned)__builtin_popcountll(cm));
            base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
            const unsigned slot = base + (unsigned)__builtin_popcountll(cm & (((unsigned long long)1 << lane) - 1ULL));
            if (c && slot < QCX_MEAS_CAND_CAP) cands->list[slot] = i;
        }
    }
    const unsigned long long nz = __ballot(!zero);
    MeasBlock g; g.S = 0; g.meta = MEAS_ALLZERO; g.pad = 0;
    if (nz) {
        const int e_ref = __builtin_amdgcn_readlane((int)(m.meta & 0x7ffu), __builtin_ctzll(nz));
        const bool bad = !zero && ((m.meta & (MEAS_TIE | MEAS_BIG | MEAS_EUNK)) || (int)(m.meta & 0x7ffu) != e_ref);
        unsigned long long tot = zero ? 0ULL : (unsigned long long)m.S;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tot += __shfl_down(tot, o, 64);
        tot = readlane_u64(tot, 0);
        if (tot > ((uint64_t)1 << 54)) tot = (uint64_t)1 << 54;
        g.S = tot;
        g.meta = (uint32_t)e_ref | (__ballot(bad) ? (uint32_t)MEAS_EUNK : 0u);
    }
    if (lane == 0) outg[blockIdx.x] = g;
}

// exact scan of one record.  Batches of 1024 amplitudes (16 per lane, the next batch's loads in flight meanwhile): when a
// whole batch has no tie / oversized element and stays inside the binade and below r, it is ONE integer addition (one
// wave reduction).  Otherwise the longest prefix of its 16 groups of 64 for which that holds is found by bisection (the sums
// are monotone), the one group in which something happens runs the strictly sequential chain, and the rest of the batch
// starts over under the binade the chain ended in.
__device__ __forceinline__ bool meas_int_value(double cum, double r, unsigned long long inc, uint32_t fl, double &cn)
{
    // all lanes: inc = this lane's integer increments under the binade of cum, fl = its flags.  true: cn = the exact running
    // sum after them (every addition stayed inside the binade and below r)
    const uint64_t cb = (uint64_t)__double_as_longlong(cum);
    const int ec = (int)((cb >> 52) & 0x7ff);
    if (ec == 0 || ec == 0x7ff) return false;
    if (__ballot(fl != 0) != 0ULL) return false;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) inc += __shfl_down(inc, o, 64);
    const uint64_t tot = readlane_u64(inc, 0);                                  // <= 1024 increments < 2^53 each: no overflow
    const uint64_t Kn = ((cb & 0xfffffffffffffULL) | ((uint64_t)1 << 52)) + tot;
    if (Kn >= ((uint64_t)1 << 53)) return false;
    cn = __longlong_as_double((long long)(((uint64_t)ec << 52) | (Kn & 0xfffffffffffffULL)));
    return !(cn >= r);
}

__device__ __forceinline__ bool wave_exact_block(const amp_t *__restrict__ amp, uint64_t first, uint64_t len,
                                                 double &cum, double r, uint64_t *hit_index, double *hit_cum)
{
    const unsigned lane = threadIdx.x & 63u;
    constexpr int G = 16;                                   // groups of 64 per batch
    double nx[G];
#pragma unroll
    for (int g = 0; g < G; g++) { const uint64_t o = (uint64_t)g * 64 + lane; nx[g] = 0.0; if (o < len) nx[g] = prob_of(amp[first + o]); }
    for (uint64_t base0 = 0; base0 < len; base0 += 64 * G) {
        double pv[G];
#pragma unroll
        for (int g = 0; g < G; g++) pv[g] = nx[g];
#pragma unroll
        for (int g = 0; g < G; g++) {                       // prefetch the next batch
            const uint64_t o = base0 + 64 * G + (uint64_t)g * 64 + lane;
            nx[g] = 0.0;
            if (o < len) nx[g] = prob_of(amp[first + o]);
        }
        int a = 0;                                          // groups [0, a) of the batch are done
        const int gmax = (int)min((uint64_t)G, (len - base0 + 63) / 64);
        while (a < gmax) {
            // this lane's increments of the groups still to do, under the binade the running sum is in now
            const int ec = (int)(((uint64_t)__double_as_longlong(cum) >> 52) & 0x7ff);
            uint64_t inc[G]; uint32_t fl[G];
#pragma unroll
            for (int g = 0; g < G; g++) {
                const uint64_t pb = (uint64_t)__double_as_longlong(pv[g]);
                uint32_t f1 = 0;
                const uint64_t i1 = meas_inc(pb, ec, f1);
                inc[g] = pb ? i1 : 0; fl[g] = pb ? f1 : 0u;
            }
            auto value = [&](int lo, int hi, double &cn) {  // the groups [lo, hi) as one integer addition
                unsigned long long sI = 0; uint32_t sF = 0;
#pragma unroll
                for (int g = 0; g < G; g++) { const bool in = g >= lo && g < hi; sI += in ? inc[g] : 0; sF |= in ? fl[g] : 0u; }
                return meas_int_value(cum, r, sI, sF, cn);
            };
            double cn = cum;
            int take = a;                                   // groups [a, take) can be taken at once
            if (!(cum >= r)) {
                if (value(a, gmax, cn)) take = gmax;
                else {
                    int lo = a, hi = gmax - 1;              // the longest good prefix ends in [lo, hi]
                    double cbest = cum;
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        double c2;
                        if (value(a, mid, c2)) { lo = mid; cbest = c2; } else hi = mid - 1;
                    }
                    take = lo; cn = cbest;
                }
            }
            if (take > a) { cum = cn; a = take; }
            if (a >= gmax) break;
            // group a: the strictly sequential chain
            double p = pv[0];                               // pv[a] without a run-time register index
#pragma unroll
            for (int q = 1; q < G; q++) p = (q == a) ? pv[q] : p;
            const uint64_t base = base0 + (uint64_t)a * 64;
            double run = cum;
#pragma unroll
            for (int jj = 0; jj < 64; jj++) {
                const double pj = readlane_f64(p, jj);
                run = run + ((int)lane >= jj ? pj : 0.0);
            }
            const bool hit = (base + lane < len) && (run >= r);
            const unsigned long long m = __ballot(hit);
            if (m) {
                const int firstl = __builtin_ctzll(m);
                *hit_index = first + base + (uint64_t)firstl;
                *hit_cum = readlane_f64(run, firstl);
                return true;
            }
            cum = readlane_f64(run, 63);
            a++;
        }
    }
    return false;
}

struct MeasLevels {
    const MeasBlock *lv[5];          // lv[0]: the records, lv[L]: sums of 64^L consecutive records
    unsigned n[5];
    int top;                         // highest level present
};

// (Round 5 staged the upper levels of the tree in LDS for the walk: no change, 3.71 against 3.72 ms on a dense n = 30 state --
// the ~30 us per event are spent in the exact rescans of the record the event lies in and in the steps' arithmetic on ONE wave,
// not in the latency of the level reads.  Not kept.)
// resume: what k_meas_fast (below) left -- nothing to do (state 0), or "go on at record b with the exact running sum cum"; nullptr:
// the whole scan is this kernel's
struct MeasResume { uint32_t state, slow; uint64_t b; double cum; };

// ENDS (the sampling scan, K4d): every record this kernel redoes exactly leaves its exact running sum at its end in ends[record]
template <bool ENDS>
__global__ __launch_bounds__(64) void k_meas_walk(const amp_t *__restrict__ amp, uint64_t count, MeasLevels T,
                                                  double cum_in, double r, MeasureOut *out, unsigned *stats, unsigned rlog, const MeasResume *resume,
                                                  MeasCands *cands, meas_slot_t *look, unsigned nslots, double *ends)
{
    const unsigned lane = threadIdx.x;
    const unsigned n0 = T.n[0];
    if (look) for (unsigned k = lane; k < nslots; k += 64u) look[k] = ~0ULL;      // (a scan without a groups launch: at most 34 slots)
    // the last kernel of a scan leaves the look-back's ticket and the candidate count at zero for the next scan (two memset
    // launches less per measurement: ~9 us of the ~100 an n = 20 attempt takes; the host falls back to memsets after a failed call)
    if (lane == 0) { cands->count = 0u; cands->ticket[0] = cands->ticket[1] = cands->ticket[2] = cands->ticket[3] = 0u; }
    double cum = cum_in;
    unsigned slow = 0;
    uint64_t b = 0;                                   // next record
    if (resume) {
        if (resume->state == 0u) return;
        b = resume->b; cum = resume->cum; slow = resume->slow;
    }
    int cap = T.top;                                  // highest level the next step may use
    uint64_t hi = 0; double hc = 0.0;
    // r already reached before the first addition (Q:289 with cum_0 >= cum_in): the first examined element is the answer
    if (b == 0 && cum_in >= r) {
        const uint64_t len = min((uint64_t)1 << rlog, count);
        slow++;
        if (wave_exact_block(amp, 0, len, cum, r, &hi, &hc)) {
            if (lane == 0) { out->found = 1; out->index = hi; out->cum = hc; if (stats) { stats[0] = slow; stats[1] = n0; } }
            return;
        }
        if (ENDS && lane == 0) ends[0] = cum;
        b = 1;
    }
    while (b < n0) {
        int L = 0;
        while (L < cap && (b & (((uint64_t)1 << (6 * (L + 1))) - 1)) == 0) L++;       // the highest level b is aligned to
        const MeasBlock *rec = T.lv[L];
        const unsigned nL = T.n[L];
        const unsigned shift = 6u * (unsigned)L;
        const uint64_t i0 = b >> shift;
        const unsigned lim = L == T.top ? 64u : 64u - (unsigned)(i0 & 63u);       // up to the next boundary of the level above
        MeasBlock mine; mine.S = 0; mine.meta = MEAS_ALLZERO; mine.pad = 0;
        if (lane < lim && i0 + lane < nL) mine = rec[i0 + lane];
        const uint64_t cb = (uint64_t)__double_as_longlong(cum);
        const int ec = (int)((cb >> 52) & 0x7ff);
        const bool ecok = ec != 0 && ec != 0x7ff;
        const bool zero = (mine.meta & MEAS_ALLZERO) != 0;
        const bool plain = zero || (ecok && !(mine.meta & (MEAS_TIE | MEAS_BIG | MEAS_EUNK)) && (int)(mine.meta & 0x7ffu) == ec);
        // inclusive sums of the increments over the lanes (saturated entries stay below 2^54 each: no overflow in 64 of them)
        unsigned long long inc = zero ? 0ULL : (unsigned long long)mine.S;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_up(inc, o, 64);
            if ((int)lane >= o) inc += up;
        }
        const uint64_t Kn = ((cb & 0xfffffffffffffULL) | ((uint64_t)1 << 52)) + inc;
        bool ok = plain && lane < lim;
        double cn = cum;                                 // the exact running sum through this lane's entry, if ok
        if (ok && (!zero || inc != 0)) {
            // (an all-zero entry adds nothing: its value is the one through the last non-zero lane before it)
            ok = ecok && Kn < ((uint64_t)1 << 53);
            if (ok) { cn = __longlong_as_double((long long)(((uint64_t)ec << 52) | (Kn & 0xfffffffffffffULL))); ok = !(cn >= r); }
        }
        const unsigned long long bad = ~__ballot(ok);
        const unsigned adv = bad ? (unsigned)__builtin_ctzll(bad) : 64u;        // entries taken in this step (monotone sums: a good lane validates all before it)
        if (adv) { cum = readlane_f64(cn, (int)adv - 1); b += (uint64_t)adv << shift; }
        if (adv >= lim) { cap = T.top; continue; }
        if (L > 0) { cap = L - 1; continue; }                                    // the entry at b needs a closer look
        // level 0: record b the slow way
        slow++;
        const uint64_t first = b << rlog;
        if (first >= count) break;
        const uint64_t len = min((uint64_t)1 << rlog, count - first);
        if (wave_exact_block(amp, first, len, cum, r, &hi, &hc)) {
            if (lane == 0) { out->found = 1; out->index = hi; out->cum = hc; if (stats) { stats[0] = slow; stats[1] = n0; } }
            return;
        }
        if (ENDS && lane == 0) ends[b] = cum;
        b++;
        cap = T.top;
    }
    if (lane == 0) { out->found = 0; out->index = 0; out->cum = cum; if (stats) { stats[0] = slow; stats[1] = n0; } }
}

// ---------------------------------------------------------------------------
// K4c, step 3a (round 5): the events of the scan WITHOUT the one-wave tree walk.  On a dense state the walk above spends ~34 us per
// record it has to redo (a binade crossing every time the running sum doubles: 32 of them at n = 30, 1.1 ms next to a 2.8 ms read)
// -- the descent to the record and back up, a dependent load per level, and the redo itself, all on one wave.  But WHERE the
// events are is known beforehand from the approximate prefixes: k_meas_groups lists the flagged records and both sides of
// every change of the binade guess (MeasCands).  One workgroup of 8 waves takes the list in index order, candidate k on wave
// k mod 8, in two phases:
//   parallel (no dependence on the running sum): the integer sum of the stretch of plain records between candidate k-1 and
//     candidate k -- straight from the tree: at most 63 entries at either end per level, every address known up front, all
//     loads in flight together -- and the candidate's own amplitudes: lane l keeps 2^rlog / 64 CONSECUTIVE probabilities in
//     registers, with their integer increments under the stretch's binade and the next one;
//   serial (wave k waits for wave k-1's exact running sum in LDS): validate the stretch against it (same binade, no overflow,
//     below r), then the record: a prefix scan of the lanes' increments finds the first lane in which something happens
//     (crossing, tie, oversized element, r); THAT lane adds its few probabilities one by one -- the reference's own
//     additions, no shuffles -- and the lanes behind it go on under the binade it ended in.  About a microsecond.
// Every decision is validated against the exact running sum exactly as in the walk, so the index is the reference's for any
// input; whatever does not go as the list predicts (a stretch that fails, more than QCX_MEAS_CAND_CAP candidates, r reached
// before the first addition) is handed to k_meas_walk with the exact state (MeasResume) -- slower, same result.
// ---------------------------------------------------------------------------
struct MeasStretch { uint64_t tot; int es; bool ok; };          // es = -1: nothing but zeros

__device__ __forceinline__ void meas_stretch_take(const MeasBlock &m, bool valid, MeasStretch &st)
{
    const bool zero = !valid || (m.meta & MEAS_ALLZERO) != 0;
    const unsigned long long nz = __ballot(!zero);
    if (!nz) return;
    if (st.es < 0) st.es = __builtin_amdgcn_readlane((int)(m.meta & 0x7ffu), __builtin_ctzll(nz));
    const bool bad = !zero && ((m.meta & (MEAS_TIE | MEAS_BIG | MEAS_EUNK)) || (int)(m.meta & 0x7ffu) != st.es);
    if (__ballot(bad)) st.ok = false;
    unsigned long long t = zero ? 0ULL : (unsigned long long)m.S;                  // <= 2^54 each
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    st.tot += readlane_u64(t, 0);                                                  // <= 10 x 64 entries: no overflow
}

// the records [a, b) as ONE integer addition, from the tree (every load issued before the first is used)
__device__ __forceinline__ MeasStretch meas_stretch(const MeasLevels &T, uint64_t a, uint64_t b)
{
    const unsigned lane = threadIdx.x & 63u;
    MeasBlock mL[5], mR[5];
    bool vL[5], vR[5];
    uint64_t ua = a, ub = b;
#pragma unroll
    for (int L = 0; L < 5; L++) {
        vL[L] = vR[L] = false;
        mL[L].S = mR[L].S = 0; mL[L].meta = mR[L].meta = MEAS_ALLZERO; mL[L].pad = mR[L].pad = 0;
        if (L > T.top || ua >= ub) continue;
        if (L == T.top) {                               // (at most 64 entries up here)
            vL[L] = lane < ub - ua;
            if (vL[L]) mL[L] = T.lv[L][ua + lane];
            ua = ub;
            continue;
        }
        const uint64_t lb = min(ub, (ua + 63u) & ~(uint64_t)63);          // up to the next group boundary
        vL[L] = lane < lb - ua;
        if (vL[L]) mL[L] = T.lv[L][ua + lane];
        if (lb < ub) {
            const uint64_t ra = ub & ~(uint64_t)63;                         // >= lb: the whole groups in between belong to the level above
            vR[L] = lane < ub - ra;
            if (vR[L]) mR[L] = T.lv[L][ra + lane];
            ua = lb >> 6; ub = ra >> 6;
        } else ua = ub;
    }
    MeasStretch st; st.tot = 0; st.es = -1; st.ok = true;
#pragma unroll
    for (int L = 0; L < 5; L++) { meas_stretch_take(mL[L], vL[L], st); meas_stretch_take(mR[L], vR[L], st); }
    return st;
}

// this lane's `per` consecutive probabilities as one integer increment under binade e (saturated), and their flags
__device__ __forceinline__ void meas_lane_inc(const double (&p)[32], unsigned per, int e, uint64_t &S, uint32_t &fl)
{
    S = 0; fl = 0;
#pragma unroll
    for (unsigned j = 0; j < 32; j++) {
        if (j < per) {
            const uint64_t pb = (uint64_t)__double_as_longlong(p[j]);
            uint32_t f1 = 0;
            const uint64_t i1 = meas_inc(pb, e, f1);
            S += pb ? i1 : 0; fl |= pb ? f1 : 0u;
        }
    }
    if (S > ((uint64_t)1 << 54)) S = (uint64_t)1 << 54;
}

// one record, exactly, from the exact running sum cum (< r on entry).  true: r was reached at *hit_index; false: cum = the running sum behind it
__device__ __forceinline__ bool meas_record_exact(const double (&p)[32], unsigned per, uint64_t first, double &cum, double r,
                                                  int eA, uint64_t SA, uint32_t flA, int eB, uint64_t SB, uint32_t flB,
                                                  uint64_t *hit_index, double *hit_cum)
{
    const unsigned lane = threadIdx.x & 63u;
    unsigned done = 0;                                   // lanes [0, done) are behind us
    while (done < 64u) {
        const uint64_t cb = (uint64_t)__double_as_longlong(cum);
        const int ec = (int)((cb >> 52) & 0x7ff);
        const bool ecok = ec != 0 && ec != 0x7ff;
        uint64_t S = 0; uint32_t fl = MEAS_EUNK;
        if (ecok) {
            if (ec == eA) { S = SA; fl = flA; }
            else if (ec == eB) { S = SB; fl = flB; }
            else meas_lane_inc(p, per, ec, S, fl);
        }
        const bool in = lane >= done;
        unsigned long long inc = in ? (unsigned long long)S : 0ULL;           // <= 2^54 each: no overflow over 64 lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_up(inc, o, 64);
            if ((int)lane >= o) inc += up;
        }
        const unsigned long long flagged = __ballot(in && fl != 0u);
        const unsigned firstfl = flagged ? (unsigned)__builtin_ctzll(flagged) : 64u;
        const uint64_t Kn = ((cb & 0xfffffffffffffULL) | ((uint64_t)1 << 52)) + inc;
        bool ok = in && ecok && lane < firstfl && Kn < ((uint64_t)1 << 53);
        double cn = cum;
        if (ok) { cn = __longlong_as_double((long long)(((uint64_t)ec << 52) | (Kn & 0xfffffffffffffULL))); ok = !(cn >= r); }
        const unsigned long long bad = ~__ballot(ok) & ~(done ? (((unsigned long long)1 << done) - 1ULL) : 0ULL);
        const unsigned L = bad ? (unsigned)__builtin_ctzll(bad) : 64u;       // monotone sums: a good lane validates all before it
        if (L > done) cum = readlane_f64(cn, (int)L - 1);
        if (L >= 64u) break;
        // lane L: the reference's own additions, one by one (every lane runs them on its own numbers; lane L's count)
        double run = cum, hc = 0.0;
        int hj = -1;
#pragma unroll
        for (unsigned j = 0; j < 32; j++) {
            if (j < per) {
                run = run + p[j];
                if (hj < 0 && run >= r) { hj = (int)j; hc = run; }
            }
        }
        const int hjL = __builtin_amdgcn_readlane(hj, (int)L);
        if (hjL >= 0) {
            *hit_index = first + (uint64_t)L * per + (uint64_t)hjL;
            *hit_cum = readlane_f64(hc, (int)L);
            return true;
        }
        cum = readlane_f64(run, (int)L);
        done = L + 1u;
    }
    return false;
}

template <bool ENDS>      // ENDS: as in k_meas_walk, the exact running sum at the end of every candidate record goes to ends[record]
__global__ __launch_bounds__(512) void k_meas_fast(const amp_t *__restrict__ amp, uint64_t count, MeasLevels T, double cum_in, double r,
                                                   MeasureOut *out, unsigned *stats, unsigned rlog, const MeasCands *cands,
                                                   MeasResume *resume, unsigned dbg, double *ends)
{
    __shared__ unsigned s_raw[QCX_MEAS_CAND_CAP], s_sorted[QCX_MEAS_CAND_CAP + 1];
    __shared__ unsigned long long s_cum[QCX_MEAS_CAND_CAP + 1];
    __shared__ unsigned s_flag[QCX_MEAS_CAND_CAP + 1];
    __shared__ unsigned s_stop;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const unsigned n0 = T.n[0], ncand = cands->count;
    if (ncand > QCX_MEAS_CAND_CAP || cum_in >= r) {                 // (uniform) not this kernel's case: the walk takes everything
        if (threadIdx.x == 0) { resume->state = 1u; resume->slow = 0u; resume->b = 0; resume->cum = cum_in; }
        return;
    }
    for (unsigned t = threadIdx.x; t < ncand; t += blockDim.x) s_raw[t] = cands->list[t];
    for (unsigned t = threadIdx.x; t <= ncand; t += blockDim.x) s_flag[t] = 0u;
    if (threadIdx.x == 0) s_stop = 0u;
    __syncthreads();
    for (unsigned t = threadIdx.x; t < ncand; t += blockDim.x) {   // rank sort (distinct values)
        const unsigned v = s_raw[t];
        unsigned rank = 0;
        for (unsigned j = 0; j < ncand; j++) rank += s_raw[j] < v ? 1u : 0u;
        s_sorted[rank] = v;
    }
    __syncthreads();
    const unsigned per = (1u << rlog) >> 6;                           // 4 .. 32 probabilities per lane
    // (no workgroup barrier below: waves leave at different times)
    for (unsigned k = wave; k <= ncand; k += nwaves) {                // k = ncand: the stretch behind the last candidate
        const uint64_t a = k ? (uint64_t)s_sorted[k - 1u] + 1u : 0u;
        const bool has_rec = k < ncand;
        const uint64_t b = has_rec ? (uint64_t)s_sorted[k] : (uint64_t)n0;
        // ---- parallel phase -------------------------------------------------------------------------------------------------
        const MeasStretch st = meas_stretch(T, a, b);
        double p[32];
        const uint64_t first = b << rlog;
        int eA = -1, eB = -1;
        uint64_t SA = 0, SB = 0; uint32_t flA = 0, flB = 0;
        if (has_rec) {
#pragma unroll
            for (unsigned j = 0; j < 32; j++) {
                p[j] = 0.0;
                if (j < per) { const uint64_t i = first + (uint64_t)lane * per + j; if (i < count) p[j] = prob_of(amp[i]); }
            }
            eA = st.es >= 0 ? st.es : (int)(T.lv[0][b].meta & 0x7ffu);     // the binade the record most likely starts in
            if (eA > 0 && eA < 0x7fe) {
                eB = eA + 1;
                meas_lane_inc(p, per, eA, SA, flA);
                meas_lane_inc(p, per, eB, SB, flB);
            } else eA = -1;
        } else {
#pragma unroll
            for (unsigned j = 0; j < 32; j++) p[j] = 0.0;
        }
        // ---- serial phase: the exact running sum behind candidate k - 1 ------------------------------------------------------
        double cum = cum_in;
        if (k) {
            unsigned f = 0;
            while (true) {
                f = __hip_atomic_load(&s_flag[k - 1u], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (f || __hip_atomic_load(&s_stop, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
                __builtin_amdgcn_s_sleep(1);
            }
            if (!f) return;                                           // somebody before us finished the scan (or handed it over)
            cum = __longlong_as_double((long long)__hip_atomic_load(&s_cum[k - 1u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        }
        bool fail = (dbg & 2u) && k == 2u;                            // (diagnostics: hand over at the third candidate)
        // the stretch [a, b): plain records under the binade of cum, no overflow, below r
        if (!fail && st.es >= 0) {
            const uint64_t cb = (uint64_t)__double_as_longlong(cum);
            const int ec = (int)((cb >> 52) & 0x7ff);
            const uint64_t Kn = ((cb & 0xfffffffffffffULL) | ((uint64_t)1 << 52)) + st.tot;
            if (!st.ok || ec == 0 || ec == 0x7ff || ec != st.es || Kn >= ((uint64_t)1 << 53)) fail = true;
            else {
                const double cn = __longlong_as_double((long long)(((uint64_t)ec << 52) | (Kn & 0xfffffffffffffULL)));
                if (cn >= r) fail = true; else cum = cn;
            }
        } else if (!fail && !st.ok) fail = true;
        if (fail) {                                                   // the walk goes on from the start of the stretch
            if (lane == 0) {
                resume->state = 1u; resume->slow = k; resume->b = a; resume->cum = cum;
                __hip_atomic_store(&s_stop, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            return;
        }
        if (has_rec) {
            uint64_t hi = 0; double hc = 0.0;
            if (meas_record_exact(p, per, first, cum, r, eA, SA, flA, eB, SB, flB, &hi, &hc)) {
                if (lane == 0) {
                    out->found = 1; out->index = hi; out->cum = hc;
                    if (stats) { stats[0] = k + 1u; stats[1] = n0; }
                    resume->state = 0u;
                    __hip_atomic_store(&s_stop, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                return;
            }
            if (lane == 0) {
                if (ENDS) ends[b] = cum;
                __hip_atomic_store(&s_cum[k], (unsigned long long)__double_as_longlong(cum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_store(&s_flag[k], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        } else if (lane == 0) {                                       // the end of the records: r was never reached
            out->found = 0; out->index = 0; out->cum = cum;
            if (stats) { stats[0] = ncand; stats[1] = n0; }
            resume->state = 0u;
        }
    }
}

// ---------------------------------------------------------------------------
// K4d  many shots from ONE state, not collapsed (qcx_sample_states, DESIGN s4.5c).  The running sum is monotone (fl(x + p) with
// p >= 0 never decreases), so the reference's answer for a draw r lies in the first RECORD whose exact end sum reaches r, and
// that record alone, redone from its exact start, gives the index.  So the state is read once for all shots:
//   1. the K4c scan run to the end (r = +inf, as qcx_total_probability runs it) with ENDS: every record k_meas_fast / k_meas_walk
//      redo exactly (an EVENT: binade crossing, tie, oversized element, wrong guess, start of the sum) leaves its exact end
//      sum in ends[];  every other record is PLAIN: the scan validated it as "all zero, or no flag and guessed in the binade
//      the exact running sum is in, with no overflow", so its increment S (MeasBlock) is an exact integer count of that
//      binade's ulp -- the K4 argument above;
//   2. k_samp_chunks / k_samp_chunk_scan / k_samp_fill: a segmented scan over the records gives every plain record its exact end
//      = (exact end of the last event before it) + (integer sum of the plain S since) x ulp, assembled in the bits (the
//      integer significand + the sum, the exponent kept).  What cannot be assembled so (no event before a non-zero plain
//      record, a carry out of the binade, a non-finite end) raises `bad`, and every shot then falls back;
//   3. k_sample_shots: one wave per shot: a 64-way search of ends[] (3-4 steps at 2^19 records), then wave_exact_block over that
//      one record from its exact start, with r -- the reference's own additions where something happens.  A record that does
//      not reach r after all (it cannot: the ends are exact) is reported as QCX_SAMP_FALLBACK, never guessed.
// k_sample_seq is step 1 for registers the single-wave scan takes (below meas_min_log2): it stores the exact running sum at the
// end of every record of 2^elog amplitudes (elog = 0: every amplitude), step 2 is then empty.
// ---------------------------------------------------------------------------
#define QCX_SAMP_NOTFOUND (~0ULL)               // the sum never reaches r before the bound: the reference's fall-through index
#define QCX_SAMP_FALLBACK (~0ULL - 1ULL)        // the fast path cannot vouch for this shot: the host runs the exact scan for it
#define QCX_SAMP_PER 16u                        // records per thread in the segmented scan; 256 threads: 4096 records per chunk
#define QCX_SAMP_CHUNK (256u * QCX_SAMP_PER)

__global__ __launch_bounds__(64) void k_sample_seq(const amp_t *__restrict__ amp, uint64_t count, double cum_in, unsigned elog, double *ends)
{
    const unsigned lane = threadIdx.x;
    const uint64_t emask = ((uint64_t)1 << elog) - 1;
    double cum = cum_in;
    for (uint64_t base = 0; base < count; base += 64) {
        const uint64_t i = base + lane;
        const double p = i < count ? prob_of(amp[i]) : 0.0;
        double run = cum;
#pragma unroll
        for (int j = 0; j < 64; j++) {                       // the chain of k_measure_scan: lane k ends holding the sum through element k
            const double pj = readlane_f64(p, j);
            run = run + ((int)lane >= j ? pj : 0.0);
        }
        if (i < count && (((i + 1) & emask) == 0 || i + 1 == count)) ends[i >> elog] = run;
        cum = readlane_f64(run, 63);
    }
}

struct SampCarry { uint64_t E, s, ev; };       // ev: a record with an exact end E (bits) lies behind; s: plain increments since (saturated)

__device__ __forceinline__ SampCarry samp_combine(const SampCarry &a, const SampCarry &b)
{
    if (b.ev) return b;
    SampCarry c = a;
    c.s = a.s + b.s;                                        // both <= 2^60: no overflow
    if (c.s > ((uint64_t)1 << 60)) c.s = (uint64_t)1 << 60;
    return c;
}

__device__ __forceinline__ SampCarry samp_item(const MeasBlock *__restrict__ blk, const double *ends, uint64_t b)
{
    SampCarry c;
    const uint64_t eb = (uint64_t)__double_as_longlong(ends[b]);
    if (eb != ~0ULL) { c.ev = 1; c.E = eb; c.s = 0; }      // (all ones: not redone by the scan, a plain record)
    else {
        const MeasBlock m = blk[b];
        c.ev = 0; c.E = 0; c.s = (m.meta & MEAS_ALLZERO) ? 0 : (m.S > ((uint64_t)1 << 60) ? (uint64_t)1 << 60 : m.S);
    }
    return c;
}

// the exact running sum a carry stands for; false: it cannot be assembled (the fast path must not answer)
__device__ __forceinline__ bool samp_value(const SampCarry &c, double cum_in, double &v)
{
    if (c.s == 0) {
        v = c.ev ? __longlong_as_double((long long)c.E) : cum_in;
        return v >= 0.0 && v < __builtin_inf();
    }
    if (!c.ev || (c.E >> 63)) return false;
    const uint64_t ex = (c.E >> 52) & 0x7ff;
    if (ex == 0 || ex == 0x7ff) return false;
    const uint64_t K = ((c.E & 0xfffffffffffffULL) | ((uint64_t)1 << 52)) + c.s;
    if (K >= ((uint64_t)1 << 53)) return false;
    v = __longlong_as_double((long long)((ex << 52) | (K & 0xfffffffffffffULL)));
    return true;
}

// this thread's QCX_SAMP_PER records folded into one carry
__device__ __forceinline__ SampCarry samp_thread_fold(const MeasBlock *__restrict__ blk, const double *ends, uint64_t b0, uint64_t nrec)
{
    SampCarry c; c.E = 0; c.s = 0; c.ev = 0;
    for (unsigned k = 0; k < QCX_SAMP_PER; k++) if (b0 + k < nrec) c = samp_combine(c, samp_item(blk, ends, b0 + k));
    return c;
}

// exclusive scan of one carry per thread over a workgroup of 256 (Hillis-Steele in LDS); *total = the whole workgroup's
__device__ __forceinline__ SampCarry samp_block_excl(SampCarry mine, SampCarry *sh, SampCarry *total)
{
    const unsigned t = threadIdx.x;
    sh[t] = mine;
    __syncthreads();
    for (unsigned o = 1; o < 256u; o <<= 1) {
        SampCarry v = sh[t];
        if (t >= o) v = samp_combine(sh[t - o], v);
        __syncthreads();
        sh[t] = v;
        __syncthreads();
    }
    SampCarry ex; ex.E = 0; ex.s = 0; ex.ev = 0;
    if (t) ex = sh[t - 1];
    *total = sh[255];
    return ex;
}

__global__ __launch_bounds__(256) void k_samp_chunks(const MeasBlock *__restrict__ blk, const double *ends, uint64_t nrec, SampCarry *chunk_tot)
{
    __shared__ SampCarry sh[256];
    const uint64_t b0 = (uint64_t)blockIdx.x * QCX_SAMP_CHUNK + (uint64_t)threadIdx.x * QCX_SAMP_PER;
    SampCarry tot;
    samp_block_excl(samp_thread_fold(blk, ends, b0, nrec), sh, &tot);
    if (threadIdx.x == 0) chunk_tot[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void k_samp_chunk_scan(const SampCarry *chunk_tot, unsigned nch, SampCarry *chunk_pre)
{
    __shared__ SampCarry sh[256];
    const unsigned per = (nch + 255u) / 256u, c0 = threadIdx.x * per;
    SampCarry mine; mine.E = 0; mine.s = 0; mine.ev = 0;
    for (unsigned k = 0; k < per; k++) if (c0 + k < nch) mine = samp_combine(mine, chunk_tot[c0 + k]);
    SampCarry tot;
    SampCarry run = samp_block_excl(mine, sh, &tot);
    for (unsigned k = 0; k < per; k++) if (c0 + k < nch) { chunk_pre[c0 + k] = run; run = samp_combine(run, chunk_tot[c0 + k]); }
}

__global__ __launch_bounds__(256) void k_samp_fill(const MeasBlock *__restrict__ blk, double *ends, uint64_t nrec, const SampCarry *chunk_pre,
                                                   double cum_in, unsigned *bad)
{
    __shared__ SampCarry sh[256];
    const uint64_t b0 = (uint64_t)blockIdx.x * QCX_SAMP_CHUNK + (uint64_t)threadIdx.x * QCX_SAMP_PER;
    SampCarry tot;
    const SampCarry ex = samp_block_excl(samp_thread_fold(blk, ends, b0, nrec), sh, &tot);
    SampCarry carry = samp_combine(chunk_pre[blockIdx.x], ex);
    bool ok = true;
    for (unsigned k = 0; k < QCX_SAMP_PER; k++) {
        const uint64_t b = b0 + k;
        if (b >= nrec) break;
        const SampCarry it = samp_item(blk, ends, b);
        carry = samp_combine(carry, it);
        double v;
        const bool good = samp_value(carry, cum_in, v);
        ok = ok && good;
        if (!it.ev && good) ends[b] = v;
    }
    if (!ok) atomicOr(bad, 1u);
}

// one wave per shot.  out[s]: the index (< last_excl), QCX_SAMP_NOTFOUND or QCX_SAMP_FALLBACK
__global__ __launch_bounds__(256) void k_sample_shots(const amp_t *__restrict__ amp, uint64_t count, const double *__restrict__ ends, uint64_t nrec,
                                                      unsigned rlog, double cum_in, const double *__restrict__ rs, uint64_t nshots,
                                                      uint64_t last_excl, const unsigned *bad, uint64_t *out)
{
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t s = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (s >= nshots) return;                                        // (uniform per wave)
    const double r = rs[s];
    uint64_t res;
    if (*bad) res = QCX_SAMP_FALLBACK;
    else if (r <= 0.0) res = 0;                                     // Q:289: cum after element 0 is >= 0 >= r
    else {
        // the first record whose exact end reaches r (NaN r: none).  Invariant: the answer lies in [lo, hi], hi = nrec = none
        uint64_t lo = 0, hi = nrec;
        while (lo < hi) {
            const uint64_t step = (hi - lo + 63u) / 64u, cnt = (hi - lo) / step;     // probes lo + (l+1) step - 1, l < cnt (<= 64)
            const uint64_t pi = lo + (uint64_t)(lane + 1u) * step - 1u;
            const bool ge = lane < cnt && ends[pi] >= r;
            const unsigned long long m = __ballot(ge);
            if (m) { const uint64_t f = (uint64_t)__builtin_ctzll(m); hi = lo + (f + 1u) * step - 1u; lo += f * step; }
            else lo += cnt * step;
        }
        if (lo >= nrec) res = QCX_SAMP_NOTFOUND;
        else {
            double cum = lo ? ends[lo - 1] : cum_in;                // < r
            const uint64_t first = lo << rlog;
            const uint64_t len = min((uint64_t)1 << rlog, count - first);
            uint64_t hit = 0; double hc = 0.0;
            if (wave_exact_block(amp, first, len, cum, r, &hit, &hc)) res = hit >= last_excl ? QCX_SAMP_NOTFOUND : hit;
            else res = QCX_SAMP_FALLBACK;
        }
    }
    if (lane == 0) out[s] = res;
}

// ---------------------------------------------------------------------------
// K6  fused multi-gate pass.  A workgroup stages a TILE of 2^T amplitudes in
// LDS -- the c lowest index bits (contiguous runs of 2^c amplitudes = 16*2^c bytes) plus nh = T - c
// arbitrary higher bits hbit[0..nh) -- applies a whole list of gates to it and writes it back: one
// HBM round trip for the lot.  Every gate performs exactly the arithmetic of its stand-alone
// kernel, in the order the gates were issued, so results are bit-identical to the unfused path:
//   H on a tile bit           butterfly between LDS slots (same t0 +/- t1 + 0.0 form)
//   controlled phase          any control/target: a bit outside the tile is a per-tile constant (the gate
//                             is skipped or applies to the whole tile); consecutive phases stay in registers
//   controlled modular mult.  when the M register is inside the tile (closed form of k_camodc)
// ---------------------------------------------------------------------------
enum : uint32_t { FUSE_H = 0, FUSE_PHASE = 1, FUSE_CAMODC = 2 };

struct FuseOp {                 // 32 bytes
    uint32_t type;
    uint32_t a;                 // H: tile-local bit;  CAMODC: M
    uint64_t mask;              // PHASE: global index bits that must all be 1
    double   c, s;              // PHASE: cos, sin.   CAMODC: reinterpreted below
};
struct FuseCamExtra {           // overlays c, s of a CAMODC op (16 bytes)
    uint32_t C, d, Cd, inv;
};
struct FuseSeg { uint8_t src, dst, len, pad; };
#define QCX_MAX_SEG 16
struct FusePass {
    uint32_t nops, T, c, nh;
    int32_t  cam_ctl_local[4];  // [0]: 1 = ROUNDS form; [1]: bytes of folded-multiply tables, [2]: their record offset in ops,
                                // [3]: byte offset of the table area behind the lut in LDS
    uint8_t  hbit[16];          // global bit carried by tile-local bit c + j, ascending
    uint32_t xm_off, xm_cnt;    // LDS copy of the records' outside-tile masks: byte offset behind the lut, entries (0 = none)
    uint32_t has_cam, dbg;      // the pass holds modular multiplies (selects the kernel variant); dbg: diagnostics only (tools/experiments/probe_pass.py):
                                // bit 0 skip the gates, bit 1 skip the stores, bit 2 skip the tile fill -- results are then wrong by design
    uint32_t dg_cnt, dg_rec_off;// tolerance mode: merged diagonals of the pass (0 = none), record offset of their table area in ops
    uint32_t dg_lds_off, dg_slim;// byte offset of their LDS area behind the lut; 1: every round of the pass is a fast round; 2: radix-8 fast rounds
    double   tol_scale;         // radix-8 passes: (1/sqrt 2) ^ (Hadamards of the pass) -- the exact power of two, times M_SQRT1_2 for an odd count -- applied once when a tile is stored
    // General tile addressing (round 4).  A pass reads the tile whose local bit j is PHYSICAL index bit in_pos[j] of the input
    // buffer (ascending in j: in_pos[j] = j for the first c) and stores it where the pass's output layout puts those bits --
    // in place on the identity layout (the default: out = in), or OUT OF PLACE into the second buffer under another
    // logical -> physical map (a CHAINED pass: the host chooses the map so that the next pass reads whole contiguous tiles and
    // only this pass's stores are gathered; the last pass of a chain stores the identity layout again).  The tile NUMBER's
    // bits are spread over the free positions of the three index spaces by run-length segments: input, output, and LOGICAL
    // (the gate records test control qubits outside the tile against the logical base index).
    uint8_t  chained, nseg_in, nseg_out, nseg_lg;
    uint8_t  in_pos[16];        // physical (input) index bit of tile-local bit j
    uint8_t  st_loc[16];        // store order: the j-th lowest OUTPUT position of the tile's bits belongs to tile-local bit st_loc[j] ...
    uint8_t  st_pos[16];        // ... and is output index bit st_pos[j] (ascending in j)
    FuseSeg  seg_in[QCX_MAX_SEG], seg_out[QCX_MAX_SEG], seg_lg[QCX_MAX_SEG];
    // gen = 1: the pass does not READ its tiles: the register is a basis state that has not been written yet (lazy reset /
    // collapse), and the tile -- that state after the closed-form circuit front, see GenFront -- is generated in LDS
    uint32_t gen, gen_rec_off, gen_lds_off;
    uint32_t gen_tab_bytes;     // gen = 3: bytes of k_gen_cols' residue -> column table in LDS (at gen_lds_off behind the columns)
    // zskip = W > 0 (W = log2 of the waves per workgroup): the wave number is mapped onto the tile-local bits zb[0..W) -- bits no
    // Hadamard of the pass targets and no multiply moves -- instead of onto the highest thread bits, and a wave whose
    // amplitudes are ALL +0 skips the rounds (gates map +0 to +0: same bits).  The host asks for it behind a circuit front:
    // there only the residues of the multiply ladder's orbit are populated among the 2^M low index values (C = 21, a = 2:
    // six of 32), so whole waves of a tile hold nothing.  Correct for any state: a wave that finds a non-zero bit works.
    uint8_t  zskip, zb[3];
    uint32_t zpad;
    uint64_t zlist;             // the zb[] ascending, one per byte
    // xp_on (round 5): the LAST pass of a compact chain stores the REAL register (k_fused_x8 only): its output index is the virtual
    // register's [L-register bits][column], cb column bits; the amplitude of L-part l and column j belongs at real index
    // (l << M) | orbit[j], every other amplitude of the 2^M-block is +0 -- the pass writes all 2^M of them, 2^(M - cb) times its
    // tile, and k_expand_compact (one more read and write of the compact form) does not run.  The expanded store order: bits
    // 0 .. M-1 of a store index = the M-register value f, the bits above = the tile's store-order bits cb .. T-1;
    // xp_pos[i] / xp_loc[i] (i >= M) = REAL index bit / tile-local bit of store-index bit i; xp_colloc[b] = tile-local bit of column bit b
    uint8_t  xp_on, xp_M, xp_cb, xp_ncols;
    uint8_t  xp_pos[24], xp_loc[24], xp_colloc[4];
    uint16_t xp_orbit[16];
};

// Which tile a workgroup takes (round 5, second half).  Workgroup slot b (blockIdx, or the b-th turn of a persistent workgroup) used
// to take tile b; now the 2^s low bits of b -- under round-robin placement the XCD the workgroup runs on, for s >= 3 -- are moved
// to bit position `pos` of the tile number: t = [b's bits above s + pos][b mod 2^s][the `pos` bits of b above s].  s = bits 12-15 of
// FusePass::dbg, pos + 1 = bits 16-20 (0: on top, the per-gate kernels' "interleaved streams" of h_plan); launch_pass sets both
// (fuse_streams_log2 / fuse_streams_pos).  Why: a chained memory-bound pass stores runs of 2^c amplitudes (128 B at c = 3), and the
// tiles whose runs are NEIGHBOURS in the output are consecutive tile numbers (planner: tiles numbered by output position).  With
// t = b, eight neighbouring runs leave from eight different XCDs, i.e. through eight different L2s; with s = 3, pos = 3 one XCD
// takes the eight tiles whose runs make up 1 KiB of the output, back to back.  n = 30 fused Hadamard sweep 19.1-19.7 -> 18.0-18.4 ms
// (same box each pair), n = 28 tolerance inverse QFT 5.02 -> 4.94; the FP64-bound exact walk does not care.  The gain swings with
// pos (pos = 2, 4: none or a loss; 1, 3, 5: the gain) and needs s >= 3 (profiles/r05_streams.txt; the microbenchmark behind it,
// a pass without gates: tools/experiments/tile_shell.hip, profiles/r05_tile_shell.txt).  Which tile a workgroup takes changes
// nothing about what it does to it: same bits.
__device__ __forceinline__ uint64_t fuse_stream_tile(uint64_t b, unsigned tiles_log2, unsigned slog, unsigned pos1)
{
    const unsigned pos = pos1 ? min(pos1 - 1u, tiles_log2 - slog) : tiles_log2 - slog;
    const uint64_t r = b >> slog, sb = b & ((1u << slog) - 1u);
    return (r & (((uint64_t)1 << pos) - 1u)) | (sb << pos) | ((r >> pos) << (pos + slog));
}

// The circuit front on a basis state (K0b, BasisFront below) evaluated per TILE of the first pass behind it (round 4): the
// front's separate write pass and the first pass's read disappear.  Same closed form, same bits: after the front, the
// 2^M-block of an amplitude index i (its bits >= M) is populated iff its non-Hadamard bits equal the basis state's, and then
// holds ONE amplitude +/- v, at the residue  f = f0 * prod over the set control bits of A_g  mod C  (one modulus for the whole
// ladder, f0 < C: the products commute; anything else takes the separate write pass).  Per tile: the controls outside the
// tile give a factor from <= 5 byte-indexed tables, the 2^h combinations of the tile-local bits >= M a table built once per
// workgroup; an element then costs one LDS look-up and a compare.
struct GenFront {
    uint64_t basis;
    uint64_t fixed_out, sign_out;           // outside-tile parts of BasisFront::fixed_mask / sign_mask
    double   v;
    uint32_t M, ncam, C, f0;                // C = 0: no multiplies (every populated block holds f0)
    uint32_t cmpmask;                       // the low-M bits that must equal the residue (Hadamards on M-register bits free them)
    uint32_t lowout_mask;                   // low-M bits that lie outside the tile (taken from the tile's base index)
    uint32_t sfm, sbv;                      // slot space: which slot bits are fixed, and to what
    uint32_t h, present;                    // slot bits; which of the five byte tables hold a control
    uint8_t  slotbit[16], lowbit[16], signbit[16];      // per tile-local bit: slot bit index / low-M bit position (0xff: none) / in the sign mask
    uint8_t  camloc[64];                    // per multiply: slot bit of its control, 0xff = outside the tile (in the byte tables)
    uint32_t camA[64];
    uint16_t tabP[5][256];                  // product of the A_g whose control is a set bit of byte f of the base index, mod C
    // the COMPACT form (FusePass::gen = 3, k_gen_cols on the virtual register of a compact chain): the pass's index space is
    // [L-register bits][column number], cb column bits; column j holds the amplitudes whose M register reads orbit[j]
    uint32_t cb, ncols, sgn_slots;          // sgn_slots: which of the tile's hot bits lie in the sign mask
    uint32_t Cinv;                          // floor(2^32 / C): x mod C without a division (k_gen_cols; x < 2^32)
    uint16_t orbit[16];                     // the populated M-register values, ascending
};

// per-thread / per-k constant of the generated fill: slot bits | low bits << 12 | sign parity << 24 of a tile-local element index
__device__ __forceinline__ uint32_t gen_pack(unsigned e, const GenFront *G, unsigned T)
{
    uint32_t w = 0;
    for (unsigned j = 0; j < T; j++) {
        if (!((e >> j) & 1u)) continue;
        if (G->slotbit[j] != 0xff) w |= 1u << G->slotbit[j];
        if (G->lowbit[j] != 0xff) w |= 1u << (12u + G->lowbit[j]);
        if (G->signbit[j]) w ^= 1u << 24;
    }
    return w;
}

// once per workgroup: the slot table (residue factor of the tile-local controls, times f0; 0xffff = block not populated)
template <int BLOCK>
__device__ __forceinline__ void gen_setup(const GenFront *G, unsigned short *phot)
{
    const unsigned nslot = 1u << G->h;
    for (unsigned s = threadIdx.x; s < nslot; s += BLOCK) {
        unsigned x = G->f0;
        if ((s & G->sfm) != G->sbv) x = 0xffffu;
        else if (G->C)
            for (unsigned g = 0; g < G->ncam; g++)
                if (G->camloc[g] != 0xff && ((s >> G->camloc[g]) & 1u)) x = (x * G->camA[g]) % G->C;
        phot[s] = (unsigned short)x;
    }
}

// per tile: res[s] = the residue of slot s for this tile (0xffff: not populated), then the tile itself
template <int BLOCK, unsigned EPT>
__device__ __forceinline__ void gen_tile(const GenFront *G, amp_t *tile, const unsigned short *phot, unsigned short *res,
                                         uint64_t base, uint32_t packT, const uint32_t (&packK)[EPT])
{
    const unsigned nslot = 1u << G->h;
    const bool pop_out = (base & G->fixed_out) == (G->basis & G->fixed_out);
    for (unsigned s = threadIdx.x; s < nslot; s += BLOCK) {
        unsigned x = phot[s];
        if (!pop_out) x = 0xffffu;
        else if (x != 0xffffu && G->C) {
#pragma unroll
            for (unsigned f = 0; f < 5; f++)
                if ((G->present >> f) & 1u) x = (x * (unsigned)G->tabP[f][(unsigned)((base >> (8u * f)) & 255u)]) % G->C;
        }
        res[s] = (unsigned short)x;
    }
    __syncthreads();
    const uint32_t lowbase = (uint32_t)base & G->lowout_mask;
    const uint32_t parbase = (uint32_t)__builtin_popcountll(base & G->sign_out) & 1u;
    const double vp = G->v, vm = -G->v;
#pragma unroll
    for (unsigned k = 0; k < EPT; k++) {
        const uint32_t w = packT ^ packK[k];
        const unsigned f = res[w & 0xfffu];
        const uint32_t low = ((w >> 12) & 0xfffu) | lowbase;
        amp_t a; a.x = 0.0; a.y = 0.0;
        if (f != 0xffffu && ((low ^ f) & G->cmpmask) == 0u) a.x = (((w >> 24) ^ parbase) & 1u) ? vm : vp;
        tile[k * BLOCK + threadIdx.x] = a;
    }
}

// index with the tile number's bits deposited by segments: bits [src, src + len) of t go to [dst, dst + len)
__device__ __forceinline__ uint64_t fuse_deposit(uint64_t t, const FuseSeg *seg, unsigned nseg)
{
    uint64_t x = 0;
    for (unsigned k = 0; k < nseg; k++) x |= ((t >> seg[k].src) & (((uint64_t)1 << seg[k].len) - 1)) << seg[k].dst;
    return x;
}
// offset of a tile-local element index under a bit -> position table (linear in its bits)
__device__ __forceinline__ uint64_t fuse_spread(unsigned e, const uint8_t *pos, unsigned T)
{
    uint64_t off = 0;
    for (unsigned j = 0; j < T; j++) off |= (uint64_t)((e >> j) & 1u) << pos[j];
    return off;
}

// One controlled modular multiply on an LDS-resident tile whose low M local bits are the M register.
//   op.a    = M | (ctl_local + 1) << 8      (0 in the high part: the control is outside the tile)
//   op.mask = global-index mask of an outside control (0 if the control is tile-local)
// The destination -> source map of the permutation case (d = 1) is tabulated once per step by the first 2^M
// threads (one 32-bit modulo each) instead of one modulo per amplitude; `lut` lives behind the tile buffers.
template <int BLOCK, unsigned EPTC>
__device__ __forceinline__ void fuse_camodc_step(amp_t *tile, unsigned short *lut, const FuseOp *__restrict__ op,
                                                 uint64_t base, unsigned tsize)
{
    const uint64_t mext = op->mask;
    if ((base & mext) != mext) return;                                   // control outside the tile is 0: identity
    const unsigned M = op->a & 0xffu;
    const int ctl_local = (int)((op->a >> 8) & 0xffu) - 1;
    const FuseCamExtra X = *reinterpret_cast<const FuseCamExtra *>(&op->c);
    const unsigned blk = 1u << M, blkmask = blk - 1u;
    const bool perm = (X.d == 1);
    if (perm) {
        for (unsigned f = threadIdx.x; f < blk; f += BLOCK) lut[f] = (unsigned short)(f < X.C ? (f * X.inv) % X.C : f);
        __syncthreads();
    }
    amp_t acc[EPTC];
    bool wr[EPTC];
#pragma unroll
    for (unsigned k = 0; k < EPTC; k++) {
        wr[k] = false;
        const unsigned e = k * BLOCK + threadIdx.x;
        if (e < tsize) {
            const unsigned f = e & blkmask;
            const bool on = ctl_local < 0 || ((e >> ctl_local) & 1u);
            if (on && f < X.C) {
                amp_t s2; s2.x = 0.0; s2.y = 0.0;
                if (perm) {
                    const amp_t sv = tile[(e - f) + lut[f]];
                    s2.x += sv.x; s2.y += sv.y;
                } else if (f % X.d == 0) {
                    unsigned src = ((f / X.d) * X.inv) % X.Cd;
                    const amp_t *b = tile + (e - f);
                    for (unsigned q = 0; q < X.d; q++, src += X.Cd) { s2.x += b[src].x; s2.y += b[src].y; }
                }
                acc[k] = s2; wr[k] = true;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (unsigned k = 0; k < EPTC; k++)
        if (wr[k]) tile[k * BLOCK + threadIdx.x] = acc[k];
    __syncthreads();
}

// the gate list applied to one LDS-resident tile (shared by the plain and the pipelined pass kernels)
template <int BLOCK, int TT, unsigned EPT>
__device__ __forceinline__ void fuse_apply_ops(amp_t *tile, unsigned short *lut, const FusePass &P, const FuseOp *__restrict__ ops,
                                               uint64_t base, uint64_t off_t, const uint64_t (&off_k)[EPT],
                                               unsigned tsize, unsigned ept)
{
    unsigned i = 0;
    while (i < P.nops) {
        const uint32_t type = ops[i].type;
        if (type == FUSE_H) {
            const unsigned j = ops[i].a;
#pragma unroll
            for (unsigned k = 0; k < (EPT + 1) / 2; k++) {
                const unsigned p = k * BLOCK + threadIdx.x;
                if (p < tsize / 2) {
                    const unsigned i0 = (unsigned)insert_zero(p, j), i1 = i0 | (1u << j);
                    amp_t a = tile[i0], b = tile[i1];
                    h_butterfly(a, b);
                    tile[i0] = a; tile[i1] = b;
                }
            }
            __syncthreads();
            i++;
        } else if (type == FUSE_PHASE) {
            // a run of consecutive diagonal gates: the thread's amplitudes stay in registers for the whole run.
            // mask (global bits outside the tile) is a per-tile constant -> scalar skip; a = mask of tile-local bits
            unsigned gend = i + 1;
            while (gend < P.nops && ops[gend].type == FUSE_PHASE) gend++;
            amp_t v[EPT];
#pragma unroll
            for (unsigned k = 0; k < EPT; k++) {
                const unsigned e = k * BLOCK + threadIdx.x;
                if (k < ept && e < tsize) v[k] = tile[e];
            }
            for (unsigned o = i; o < gend; o++) {
                const uint64_t mext = ops[o].mask;                      // wave-uniform: scalar loads
                if ((base & mext) != mext) continue;
                const uint32_t mloc = ops[o].a;
                const double cc = ops[o].c, ss = ops[o].s;
#pragma unroll
                for (unsigned k = 0; k < EPT; k++) {
                    const unsigned e = k * BLOCK + threadIdx.x;
                    if (k < ept && e < tsize && (e & mloc) == mloc) {
                        amp_t w;
                        w.x = ((cc * v[k].x) - (ss * v[k].y)) + 0.0;
                        w.y = ((cc * v[k].y) + (ss * v[k].x)) + 0.0;
                        v[k] = w;
                    }
                }
            }
#pragma unroll
            for (unsigned k = 0; k < EPT; k++) {
                const unsigned e = k * BLOCK + threadIdx.x;
                if (k < ept && e < tsize) tile[e] = v[k];
            }
            __syncthreads();
            i = gend;
        } else {    // FUSE_CAMODC
            fuse_camodc_step<BLOCK, EPT>(tile, lut, ops + i, base, tsize);
            i++;
        }
    }

}

// ROUNDS form of the gate list (tiles with exactly 4 amplitudes per thread).  The host cuts the list into
// rounds; in a round every thread keeps the 4 amplitudes that differ in the round's two REGISTER BITS
// (rb0 < rb1, tile-local) in registers and applies the whole round to them:
//   H on a register bit   = butterflies between registers (two H's per LDS round trip: radix 4);
//   controlled phase      = rotate the registers the host selected (rsel: which of the 4 have the mask's
//                           register bits set), after ONE test of the remaining local bits per thread and one
//                           test of the bits outside the tile per tile.
// Same arithmetic, same order per amplitude as the per-gate kernels.  Records of a round (32 B each):
//   FUSE_ROUND   a = rb0 | rb1 << 8 | (round contains an H) << 16,  mask = records that follow (items + gates)
//   item H       type = FUSE_H    | (32 | which register bit) << 8
//   item run     type = FUSE_PRUN | (rsel | (canonicalise at the end of the run) << 4) << 8 | gates << 16  (1..64 gates)
//   gate of run  type = FUSE_PHASE | rsel << 8,  a = tile-local mask without the register bits,
//                mask = index bits outside the tile,  c, s = cos, sin
// Between rounds: FUSE_CAMRUN (folded modular multiplies) and FUSE_CAMODC (a single one) with their own layouts.
enum : uint32_t { FUSE_ROUND = 3, FUSE_CAMRUN = 5 };

__device__ __forceinline__ void rotate_amp(amp_t &v, double cc, double ss)
{
    amp_t w;
    w.x = ((cc * v.x) - (ss * v.y)) + 0.0;
    w.y = ((cc * v.y) + (ss * v.x)) + 0.0;
    v = w;
}

// A run of consecutive controlled phases that rotate the same registers (rsel).
//  * Which gates of the run act on this TILE (their controls outside the tile are all 1): lane l tests gate l
//    against the tile's base index, one ballot gives the live set, and only live gates are walked.  A skipped
//    gate costs nothing.
//  * The walk is hand-scheduled: measured, the compiler's version of this loop is bound by the scalar-ALU issue
//    port (about 20 s_* instructions per gate for mask iteration, record address, select and EXEC bookkeeping),
//    not by the FP64 work.  Here a gate costs ~9 scalar instructions: find/clear its bit, three scalar loads of
//    its record (the next gate's record is in flight while the current one is applied), a v_cmpx that masks the
//    lanes whose tile-local control bits are not all set, and the EXEC restore.
//  * A rotation is the same four products and two sums as rotate_amp, in place, without FMA.
//  * The reference's result of every rotation is canonical (its "0 + ..." turns -0 into +0).  The sign of a zero
//    never changes a later non-zero result and every zero result is canonicalised anyway, so the "+ 0.0" is
//    applied ONCE: at the end of a round that contains an H (an H touches every amplitude), otherwise at the end of
//    the run to the lanes that were rotated at least once (tch collects their EXEC masks); untouched lanes keep
//    their bits.  Same values, bit for bit, as rotate_amp per gate.
enum : uint32_t { FUSE_PRUN = 4 };

// one record = one s_load_dwordx8 into a fixed block of scalar registers (A: s[72:79], B: s[80:87]; listed as clobbers):
// dword 1 = tile-local mask, dwords 4-5 = cos, 6-7 = sin.  (Three separate loads of m, c, s cost two more instructions of the
// scalar port per gate, and this walk is bound by that port as much as by the vector one: DESIGN.md s4.)
#define QCX_RECA_M "s73"
#define QCX_RECA_C "s[76:77]"
#define QCX_RECA_S "s[78:79]"
#define QCX_RECB_M "s81"
#define QCX_RECB_C "s[84:85]"
#define QCX_RECB_S "s[86:87]"
#define QCX_LOADREC(BLK)                                             \
    "s_ff1_i32_b64 %[b], %[live]\n\t"                                \
    "s_bitset0_b64 %[live], %[b]\n\t"                                \
    "s_lshl_b32 %[b], %[b], 5\n\t"                                   \
    "s_load_dwordx8 " BLK ", %[base], %[b] offset:0x20\n\t"
#define QCX_ROT1(C, S, X, Y)                                         \
    "v_mul_f64 %[t0], " C ", %[" X "]\n\t"                          \
    "v_mul_f64 %[t1], " S ", %[" Y "]\n\t"                          \
    "v_mul_f64 %[t2], " C ", %[" Y "]\n\t"                          \
    "v_mul_f64 %[t3], " S ", %[" X "]\n\t"                          \
    "v_add_f64 %[" X "], %[t0], -%[t1]\n\t"                          \
    "v_add_f64 %[" Y "], %[t2], %[t3]\n\t"
#define QCX_ROT2(C, S, X0, Y0, X1, Y1)                               \
    "v_mul_f64 %[t0], " C ", %[" X0 "]\n\t"                         \
    "v_mul_f64 %[t1], " S ", %[" Y0 "]\n\t"                         \
    "v_mul_f64 %[t2], " C ", %[" Y0 "]\n\t"                         \
    "v_mul_f64 %[t3], " S ", %[" X0 "]\n\t"                         \
    "v_add_f64 %[" X0 "], %[t0], -%[t1]\n\t"                         \
    "v_mul_f64 %[t0], " C ", %[" X1 "]\n\t"                         \
    "v_mul_f64 %[t1], " S ", %[" Y1 "]\n\t"                         \
    "v_add_f64 %[" Y0 "], %[t2], %[t3]\n\t"                          \
    "v_mul_f64 %[t2], " C ", %[" Y1 "]\n\t"                         \
    "v_mul_f64 %[t3], " S ", %[" X1 "]\n\t"                         \
    "v_add_f64 %[" X1 "], %[t0], -%[t1]\n\t"                         \
    "v_add_f64 %[" Y1 "], %[t2], %[t3]\n\t"
#define QCX_R1(C, S, i) QCX_ROT1(C, S, "x" #i, "y" #i)
#define QCX_R2(C, S, i, j) QCX_ROT2(C, S, "x" #i, "y" #i, "x" #j, "y" #j)
// the rotations of one gate for every register selection RSEL (bit q set: amplitude register q is rotated)
#define QCX_ROTS_1(C, S)  QCX_R1(C, S, 0)
#define QCX_ROTS_2(C, S)  QCX_R1(C, S, 1)
#define QCX_ROTS_3(C, S)  QCX_R2(C, S, 0, 1)
#define QCX_ROTS_4(C, S)  QCX_R1(C, S, 2)
#define QCX_ROTS_5(C, S)  QCX_R2(C, S, 0, 2)
#define QCX_ROTS_6(C, S)  QCX_R2(C, S, 1, 2)
#define QCX_ROTS_7(C, S)  QCX_R2(C, S, 0, 1) QCX_R1(C, S, 2)
#define QCX_ROTS_8(C, S)  QCX_R1(C, S, 3)
#define QCX_ROTS_9(C, S)  QCX_R2(C, S, 0, 3)
#define QCX_ROTS_10(C, S) QCX_R2(C, S, 1, 3)
#define QCX_ROTS_11(C, S) QCX_R2(C, S, 0, 1) QCX_R1(C, S, 3)
#define QCX_ROTS_12(C, S) QCX_R2(C, S, 2, 3)
#define QCX_ROTS_13(C, S) QCX_R2(C, S, 0, 2) QCX_R1(C, S, 3)
#define QCX_ROTS_14(C, S) QCX_R2(C, S, 1, 2) QCX_R1(C, S, 3)
#define QCX_ROTS_15(C, S) QCX_R2(C, S, 0, 1) QCX_R2(C, S, 2, 3)
#define QCX_Z1(i) "v_add_f64 %[x" #i "], %[x" #i "], 0\n\t" "v_add_f64 %[y" #i "], %[y" #i "], 0\n\t"
#define QCX_ZERO_1  QCX_Z1(0)
#define QCX_ZERO_2  QCX_Z1(1)
#define QCX_ZERO_3  QCX_Z1(0) QCX_Z1(1)
#define QCX_ZERO_4  QCX_Z1(2)
#define QCX_ZERO_5  QCX_Z1(0) QCX_Z1(2)
#define QCX_ZERO_6  QCX_Z1(1) QCX_Z1(2)
#define QCX_ZERO_7  QCX_Z1(0) QCX_Z1(1) QCX_Z1(2)
#define QCX_ZERO_8  QCX_Z1(3)
#define QCX_ZERO_9  QCX_Z1(0) QCX_Z1(3)
#define QCX_ZERO_10 QCX_Z1(1) QCX_Z1(3)
#define QCX_ZERO_11 QCX_Z1(0) QCX_Z1(1) QCX_Z1(3)
#define QCX_ZERO_12 QCX_Z1(2) QCX_Z1(3)
#define QCX_ZERO_13 QCX_Z1(0) QCX_Z1(2) QCX_Z1(3)
#define QCX_ZERO_14 QCX_Z1(1) QCX_Z1(2) QCX_Z1(3)
#define QCX_ZERO_15 QCX_Z1(0) QCX_Z1(1) QCX_Z1(2) QCX_Z1(3)
// one gate: mask the lanes, rotate, restore EXEC.  A gate without tile-local conditions (its mask word is 0: the usual
// case, a phase whose target lies outside the tile) skips the two vector instructions of the lane mask and the EXEC
// round trip: the pass is bound by vector issue, the scalar compare + branch ride the other port.
#define QCX_GATE(M, ROTS)                                            \
    "s_cmp_eq_u32 " M ", 0\n\t"                                      \
    "s_cbranch_scc1 6f\n\t"                                         \
    "v_and_b32 %[t], " M ", %[p]\n\t"                                \
    "v_cmpx_eq_u32_e32 vcc, " M ", %[t]\n\t"                         \
    "s_cbranch_execz 1f\n\t"                                        \
    ROTS                                                             \
    "1:\n\t"                                                        \
    "s_mov_b64 exec, %[ex]\n\t"                                     \
    "s_branch 7f\n\t"                                               \
    "6:\n\t"                                                        \
    ROTS                                                             \
    "7:\n\t"
// H on one of the round's two register bits, in place and without the final "+ 0.0" (the round canonicalises once at
// its end): the same four products and four sums as h_butterfly
#define QCX_HBF(AX, AY, BX, BY)                                      \
    "v_mul_f64 %[t0], %[hs], %[" AX "]\n\t"                          \
    "v_mul_f64 %[t1], %[hs], %[" AY "]\n\t"                          \
    "v_mul_f64 %[t2], %[hs], %[" BX "]\n\t"                          \
    "v_mul_f64 %[t3], %[hs], %[" BY "]\n\t"                          \
    "v_add_f64 %[" AX "], %[t0], %[t2]\n\t"                          \
    "v_add_f64 %[" AY "], %[t1], %[t3]\n\t"                          \
    "v_add_f64 %[" BX "], %[t0], -%[t2]\n\t"                         \
    "v_add_f64 %[" BY "], %[t1], -%[t3]\n\t"
// all live gates of one run for register selection R (live != 0 on entry, 0 on exit); records ping-pong between
// blocks A and B; then the canonical zeros if bit 4 of rsel asks for them -- on ALL lanes of the run's registers: a gate
// kernel never meets a -0 it has not made itself (the state is canonical whenever gates run: a state written by the caller
// is canonicalised first, qcx_api.hip), so "+ 0.0" on an amplitude no gate of the run rotated changes nothing
#define QCX_RUN_BODY(R)                                              \
    QCX_LOADREC("s[72:79]")                                          \
    "2:\n\t"                                                         \
    "s_waitcnt lgkmcnt(0)\n\t"                                       \
    "s_cmp_eq_u64 %[live], 0\n\t"                                    \
    "s_cbranch_scc1 3f\n\t"                                          \
    QCX_LOADREC("s[80:87]")                                          \
    QCX_GATE(QCX_RECA_M, QCX_ROTS_##R(QCX_RECA_C, QCX_RECA_S))       \
    "s_waitcnt lgkmcnt(0)\n\t"                                       \
    "s_cmp_eq_u64 %[live], 0\n\t"                                    \
    "s_cbranch_scc1 4f\n\t"                                          \
    QCX_LOADREC("s[72:79]")                                          \
    QCX_GATE(QCX_RECB_M, QCX_ROTS_##R(QCX_RECB_C, QCX_RECB_S))       \
    "s_branch 2b\n\t"                                                \
    "3:\n\t"                                                         \
    QCX_GATE(QCX_RECA_M, QCX_ROTS_##R(QCX_RECA_C, QCX_RECA_S))       \
    "s_branch 5f\n\t"                                                \
    "4:\n\t"                                                         \
    QCX_GATE(QCX_RECB_M, QCX_ROTS_##R(QCX_RECB_C, QCX_RECB_S))       \
    "5:\n\t"                                                         \
    "s_bitcmp1_b32 %[rsel], 12\n\t"                                  \
    "s_cbranch_scc0 99f\n\t"                                         \
    QCX_ZERO_##R                                                     \
    "s_branch 99f\n\t"
// ONE asm statement for every register selection (entry 20 + R, binary dispatch on rsel & 15): with one statement
// per selection behind a C++ switch the compiler copied all four amplitudes into fresh VGPRs at every run
#define QCX_ITEM_ALL                                                 \
    /* prefetch for the NEXT item (1 + gates records further on): its header dword and its lanes' outside-tile masks */ \
    "s_lshr_b32 %[b], %[rsel], 16\n\t"                               \
    "s_add_u32 %[b], %[b], 1\n\t"                                    \
    "s_lshl_b32 %[tn], %[b], 5\n\t"                                  \
    "s_load_dword %[tn], %[base], %[tn]\n\t"                         \
    "v_lshl_add_u32 %[xa], %[b], 3, %[xa]\n\t"                       \
    "ds_read_b64 %[mn], %[xa]\n\t"                                   \
    "s_bitcmp1_b32 %[rsel], 13\n\t"                                  \
    "s_cbranch_scc1 50f\n\t"                                         \
    "s_mov_b64 %[ex], exec\n\t"                                      \
    "s_cmp_eq_u64 %[live], 0\n\t"                                    \
    "s_cbranch_scc1 99f\n\t"                                         \
    "s_bfe_u32 %[b], %[rsel], 0x40008\n\t"                           \
    "s_cmp_lt_u32 %[b], 8\n\t s_cbranch_scc1 40f\n\t"                \
    "s_cmp_lt_u32 %[b], 12\n\t s_cbranch_scc1 41f\n\t"               \
    "s_cmp_lt_u32 %[b], 14\n\t s_cbranch_scc1 42f\n\t"               \
    "s_cmp_eq_u32 %[b], 14\n\t s_cbranch_scc1 34f\n\t s_branch 35f\n\t" \
    "42:\n\t s_cmp_eq_u32 %[b], 12\n\t s_cbranch_scc1 32f\n\t s_branch 33f\n\t" \
    "41:\n\t s_cmp_lt_u32 %[b], 10\n\t s_cbranch_scc1 43f\n\t s_cmp_eq_u32 %[b], 10\n\t s_cbranch_scc1 30f\n\t s_branch 31f\n\t" \
    "43:\n\t s_cmp_eq_u32 %[b], 8\n\t s_cbranch_scc1 28f\n\t s_branch 29f\n\t" \
    "40:\n\t s_cmp_lt_u32 %[b], 4\n\t s_cbranch_scc1 44f\n\t"        \
    "s_cmp_lt_u32 %[b], 6\n\t s_cbranch_scc1 45f\n\t s_cmp_eq_u32 %[b], 6\n\t s_cbranch_scc1 26f\n\t s_branch 27f\n\t" \
    "45:\n\t s_cmp_eq_u32 %[b], 4\n\t s_cbranch_scc1 24f\n\t s_branch 25f\n\t" \
    "44:\n\t s_cmp_lt_u32 %[b], 2\n\t s_cbranch_scc1 21f\n\t s_cmp_eq_u32 %[b], 2\n\t s_cbranch_scc1 22f\n\t s_branch 23f\n\t" \
    "21:\n\t" QCX_RUN_BODY(1)  "22:\n\t" QCX_RUN_BODY(2)  "23:\n\t" QCX_RUN_BODY(3)  "24:\n\t" QCX_RUN_BODY(4)  \
    "25:\n\t" QCX_RUN_BODY(5)  "26:\n\t" QCX_RUN_BODY(6)  "27:\n\t" QCX_RUN_BODY(7)  "28:\n\t" QCX_RUN_BODY(8)  \
    "29:\n\t" QCX_RUN_BODY(9)  "30:\n\t" QCX_RUN_BODY(10) "31:\n\t" QCX_RUN_BODY(11) "32:\n\t" QCX_RUN_BODY(12) \
    "33:\n\t" QCX_RUN_BODY(13) "34:\n\t" QCX_RUN_BODY(14) "35:\n\t" QCX_RUN_BODY(15) \
    "50:\n\t"                                                        \
    "s_bitcmp1_b32 %[rsel], 8\n\t"                                   \
    "s_cbranch_scc1 51f\n\t"                                         \
    QCX_HBF("x0", "y0", "x1", "y1") QCX_HBF("x2", "y2", "x3", "y3")  \
    "s_branch 99f\n\t"                                               \
    "51:\n\t"                                                        \
    QCX_HBF("x0", "y0", "x2", "y2") QCX_HBF("x1", "y1", "x3", "y3")  \
    "99:\n\t"                                                        \
    "s_waitcnt lgkmcnt(0)\n\t"

// the four amplitudes a thread holds during a round, as eight separate doubles
struct Quad { double x0, y0, x1, y1, x2, y2, x3, y3; };

// One item of a round: an H on one of the round's register bits, or a phase run (at most 64 gates: the host cuts
// longer ones).  hdr = the item's header dword: type | code << 8 | gates << 16 with code bit 5 = H (bit 0: which
// register bit); otherwise code bits 0-3 = which amplitude registers the run rotates, bit 4 = apply the canonical
// zeros (the reference's "+ 0") to the rotated lanes at its end -- clear when the round canonicalises everything at
// its end anyway (it contains an H).  item = the item's header record, the gates of a run follow it; live = the run's
// gates whose outside-tile controls are all 1 for this tile.
// The statement also fetches what the NEXT item needs first -- its header dword (hdr_next) and this lane's entry of
// its outside-tile masks (mask_next; xaddr = LDS byte address of the current item's entry, advanced in place) -- so
// that those two latencies overlap this item's work instead of starting the next one.
// ONE asm statement for everything that touches the amplitudes inside the round's item loop: with separate
// statements (or C++ butterflies) the compiler keeps two sets of VGPRs for the four amplitudes and copies between
// them at every item, which costs more than a gate.
// The record blocks s[72:79] / s[80:87] are named registers on the clobber list.  The kernels that hold this statement are
// built for at most 7 waves per SIMD (round 5), where the blocks lie inside the allocator's budget: it works around the
// clobbers, the kernel descriptor counts them, and hipcc has nothing to warn about (tests/test_abi_and_build.py checks
// the build log and the metadata).  (Rounds 2-4 also had 8-wave builds, with the blocks beyond the allocator's budget --
// "reserved registers" -- which were no faster: 96 SGPRs admit 7 blocks of 256 threads per CU, not 8.)
__device__ __forceinline__ void fuse_round_item(Quad &q, const FuseOp *item, uint64_t live, unsigned p, uint32_t hdr,
                                                uint32_t &xaddr, uint32_t &hdr_next, uint64_t &mask_next)
{
    uint64_t ex; uint32_t bidx, tv;
    double t0, t1, t2, t3;
    const double hs = QCX_SQRT1_2;
    asm(QCX_ITEM_ALL
        : [live] "+s"(live), [ex] "=&s"(ex), [b] "=&s"(bidx), [t] "=&v"(tv),
          [x0] "+v"(q.x0), [y0] "+v"(q.y0), [x1] "+v"(q.x1), [y1] "+v"(q.y1), [x2] "+v"(q.x2), [y2] "+v"(q.y2), [x3] "+v"(q.x3), [y3] "+v"(q.y3),
          [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3),
          [tn] "=&s"(hdr_next), [mn] "=&v"(mask_next), [xa] "+v"(xaddr)
        : [base] "s"(item), [p] "v"(p), [rsel] "s"(hdr), [hs] "s"(hs)
        : "vcc", "scc", "s72", "s73", "s74", "s75", "s76", "s77", "s78", "s79", "s80", "s81", "s82", "s83", "s84", "s85", "s86", "s87");
}


// a run of consecutive permutation-type modular multiplies (gcd(A, C) = 1, same C) folded into ONE
// gather: inside a 2^M block all amplitudes share the L-register bits, so the run moves the amplitude
// of value g from  f0 = (prod of the inverses whose control is set) * g  mod C.  The product is
// walked through per-gate tables x -> x * inv_i mod C kept in LDS (camtab); pure data movement, the
// same bits as applying the gates one by one.  Returns the number of gate records behind the header.
template <int BLOCK, int TT>
__device__ __forceinline__ unsigned fuse_camrun_step(amp_t *tile, unsigned short *lut, const unsigned char *camtab,
                                                     const FuseOp *__restrict__ ops, unsigned i, uint64_t base)
{
    const unsigned cnt = ops[i].a & 0xffffu, cpad = ops[i].a >> 16;
    const unsigned char *tabs = camtab + (unsigned)ops[i].mask;
    const FuseOp *rec = ops + i + 1;
    const unsigned M = rec[0].a & 0xffu, blkmask = (1u << M) - 1u;
    const unsigned Cn = reinterpret_cast<const FuseCamExtra *>(&rec[0].c)->C;
    // The factor depends on the index only through the control bits, i.e. through the 2^M-BLOCK an amplitude
    // sits in (controls are L-register qubits, at or above M): it is walked once per block by the first
    // 2^(T-M) threads and left in LDS (the scratch behind the tile), not once per amplitude by everybody.
    unsigned char *xblk = reinterpret_cast<unsigned char *>(lut);
    for (unsigned b = threadIdx.x; b < ((1u << TT) >> M); b += BLOCK) {
        const unsigned e = b << M;
        unsigned x = 1;
        for (unsigned g = 0; g < cnt; g++) {
            const uint64_t mext = rec[g].mask;
            if ((base & mext) != mext) continue;                  // outside control is 0 for this tile
            const int cl = (int)((rec[g].a >> 8) & 0xffu) - 1;
            if (cl < 0 || ((e >> cl) & 1u)) x = tabs[g * cpad + x];
        }
        xblk[b] = (unsigned char)x;
    }
    __syncthreads();
    const float rc = 1.0f / (float)Cn;
    amp_t acc[4];
    bool wr[4];
#pragma unroll
    for (unsigned k = 0; k < 4; k++) {
        const unsigned e = k * BLOCK + threadIdx.x, f = e & blkmask;
        const unsigned x = xblk[e >> M];
        wr[k] = (x != 1u) && (f < Cn);
        if (wr[k]) {
            // (x * f) mod C for x, f < C <= 256: quotient estimate from the float reciprocal, off by at most one
            const unsigned v = x * f;
            unsigned q = (unsigned)((float)v * rc);
            int rem = (int)v - (int)(q * Cn);
            if (rem < 0) rem += (int)Cn; else if (rem >= (int)Cn) rem -= (int)Cn;
            const amp_t sv = tile[(e - f) + (unsigned)rem];
            acc[k].x = 0.0 + sv.x; acc[k].y = 0.0 + sv.y;
        }
    }
    __syncthreads();
#pragma unroll
    for (unsigned k = 0; k < 4; k++)
        if (wr[k]) tile[k * BLOCK + threadIdx.x] = acc[k];
    __syncthreads();
    return cnt;
}

// ---------------------------------------------------------------------------
// K6t  TOLERANCE MODE of the rounds form (qcx_set_fusion(reg, 2); opt-in, NOT bit-exact: amplitudes agree with the
// reference to ~1e-15, north_star allows 1e-10).  The planner merges every run of consecutive controlled phases that
// share a control qubit l into ONE diagonal (Q:682-689 applies l - M of them after each Hadamard):
//     amp[i] *= prod over the targets k with bit k of i set of (c_k + i s_k),     for every i with bit l set.
// The product splits over where the target bits live:
//     E_out(tile)        targets outside the tile: a per-tile constant.  One thread per diagonal builds it at tile start
//                        (while the LDS-DMA fill is in flight) from <= 5 tables of 256 entries indexed by the bytes of the
//                        tile's base index (global memory, L2-resident), and leaves it in LDS;
//     G0 G1 G2 (thread)  targets on tile-local bits, 4 local bits per table, 16 entries each, in LDS (768 B per diagonal);
//                        the entry for a single set bit is that bit's own factor, so the factors of the round's two
//                        register bits are read from the same tables.
// A thread then multiplies the two amplitudes whose control bit is set by F and F w(other register bit): one complex
// multiply per amplitude instead of one rotation per gate per amplitude, FMA allowed.
// Only rounds of the shape the schedule of Q:682-689 produces carry merged diagonals (FUSE_QROUND below); everywhere
// else the planner puts the original phases back, and those -- like every Hadamard outside a fast round and the modular
// multiplies -- run through the exact interpreter, same bits as in modes 0 / 1.
// ---------------------------------------------------------------------------
// The schedule of Q:682-689 gives rounds of the shape  H(x) D(x) H(y) D(y)  (x, y = the round's register bits, D(b) = a
// merged diagonal whose control is b).  The host recognises them (FUSE_QROUND: header + ONE record with two step words)
// and the kernel runs them as straight-line code: every table read of the round is issued up front, nothing is fetched
// between the butterflies.  Step word: bit 0 = the step's bit is rb1, bit 1 = a diagonal follows the H, bits 8-15 its
// slot, bits 16-18 its groups, bit 19 = the round's OTHER register bit is one of its targets; 0xffffffff = no step.
enum : uint32_t { FUSE_DIAG = 6 /* planner-side only: a merged diagonal before the rounds are formed; never reaches a kernel */, FUSE_QROUND = 7 };
struct DiagInfo {               // 48 B = 3 units of 16 B; offsets in 16-B units from the table area
    uint32_t field_off[5]; uint32_t present; uint32_t pad[2];
    double   kc, ks;            // constant factor of the diagonal: the product of the run's phases whose other qubit is a constant 1
};                              // of the view (a shard-id or slice bit): a sharded register hands such phases down with one mask bit

__device__ __forceinline__ void cmul_tol(amp_t &v, const amp_t w)        // v *= w, 2 mul + 2 fma
{
    const double nx = __builtin_fma(w.x, v.x, -(w.y * v.y));
    const double ny = __builtin_fma(w.x, v.y, w.y * v.x);
    v.x = nx; v.y = ny;
}
__device__ __forceinline__ void h_butterfly_tol(amp_t &a, amp_t &b)
{
    const double s = QCX_SQRT1_2;
    const double t0r = s * a.x, t0i = s * a.y, t1r = s * b.x, t1i = s * b.y;
    a.x = t0r + t1r;  a.y = t0i + t1i;
    b.x = t0r - t1r;  b.y = t0i - t1i;
}

// factors of one step of a fast round: F for the register whose other register bit is clear, F3 for the one where it is set
__device__ __forceinline__ void qround_factors(uint32_t s, unsigned p, unsigned rb0, unsigned rb1, const amp_t *dg, const amp_t *gtab,
                                               amp_t &F, amp_t &F3)
{
    const unsigned slot = (s >> 8) & 0xffu;
    const amp_t *G = gtab + slot * 48u;
    F = dg[slot];
    if (s & (1u << 16)) cmul_tol(F, G[p & 15u]);
    if (s & (1u << 17)) cmul_tol(F, G[16u + ((p >> 4) & 15u)]);
    if (s & (1u << 18)) cmul_tol(F, G[32u + (p >> 8)]);
    F3 = F;
    if (s & (1u << 19)) {
        const unsigned ob = (s & 1u) ? rb0 : rb1;
        cmul_tol(F3, G[16u * (ob >> 2) + (1u << (ob & 3u))]);
    }
}

// one step of a fast round on fixed registers: H between (lo0, hi0) and (lo1, hi1), then (dgl) the diagonal on the two
// amplitudes that have the step's bit set
__device__ __forceinline__ void qround_step(bool dgl, amp_t &lo0, amp_t &hi0, amp_t &lo1, amp_t &hi1, const amp_t F, const amp_t F3)
{
    h_butterfly_tol(lo0, hi0); h_butterfly_tol(lo1, hi1);
    if (dgl) { cmul_tol(hi0, F); cmul_tol(hi1, F3); }
}

// a whole fast round with the bit of each step fixed at compile time (HA / HB: the step works on rb1), from the LDS reads
// to the LDS writes: written once per combination so that which register a step touches is never a run-time choice (a
// run-time choice makes the compiler keep the four amplitudes in scratch memory and index them)
template <bool HA, bool HB>
__device__ __forceinline__ void qround_run(amp_t *tile, unsigned p, unsigned e1, unsigned e2, unsigned e3, unsigned rb0, unsigned rb1,
                                           uint32_t sA, uint32_t sB, const amp_t *dg, const amp_t *gtab)
{
    amp_t F, F3;
    F.x = F3.x = 1.0; F.y = F3.y = 0.0;
    const bool dA = (sA & 2u) != 0, two = sB != 0xffffffffu, dB = two && (sB & 2u);
    amp_t v0 = tile[p], v1 = tile[e1], v2 = tile[e2], v3 = tile[e3];
    if (dA) qround_factors(sA, p, rb0, rb1, dg, gtab, F, F3);
    if (HA) qround_step(dA, v0, v2, v1, v3, F, F3); else qround_step(dA, v0, v1, v2, v3, F, F3);
    __builtin_amdgcn_sched_barrier(0);          // (keeps the second step's table reads out of the first step's registers)
    if (two) {
        if (dB) qround_factors(sB, p, rb0, rb1, dg, gtab, F, F3);
        if (HB) qround_step(dB, v0, v2, v1, v3, F, F3); else qround_step(dB, v0, v1, v2, v3, F, F3);
    }
    tile[p] = v0; tile[e1] = v1; tile[e2] = v2; tile[e3] = v3;
}

// the same fast round on a COLUMN of k_gen_cols: the four amplitudes sit at l0 .. l3 of the column, p is their logical
// tile-local index (the table look-ups want its bits)
template <bool HA, bool HB>
__device__ __forceinline__ void qround_run_col(amp_t *col, unsigned l0, unsigned l1, unsigned l2, unsigned l3, unsigned p, unsigned rb0, unsigned rb1,
                                               uint32_t sA, uint32_t sB, const amp_t *dg, const amp_t *gtab)
{
    amp_t F, F3;
    F.x = F3.x = 1.0; F.y = F3.y = 0.0;
    const bool dA = (sA & 2u) != 0, two = sB != 0xffffffffu, dB = two && (sB & 2u);
    amp_t v0 = col[l0], v1 = col[l1], v2 = col[l2], v3 = col[l3];
    if (dA) qround_factors(sA, p, rb0, rb1, dg, gtab, F, F3);
    if (HA) qround_step(dA, v0, v2, v1, v3, F, F3); else qround_step(dA, v0, v1, v2, v3, F, F3);
    __builtin_amdgcn_sched_barrier(0);
    if (two) {
        if (dB) qround_factors(sB, p, rb0, rb1, dg, gtab, F, F3);
        if (HB) qround_step(dB, v0, v2, v1, v3, F, F3); else qround_step(dB, v0, v1, v2, v3, F, F3);
    }
    col[l0] = v0; col[l1] = v1; col[l2] = v2; col[l3] = v3;
}

// zero-wave skipping (FusePass::zskip): the element index of a thread when the wave number rides on the tile-local bits zb[]
// and the lane number on the remaining positions, ascending.  `list` = the positions to leave out of the lane number (the zb[]
// and, inside a round, its register bits), ascending, one per byte (the host sorts them: FusePass::zlist for the whole tile,
// the c field of a round's header record for a round); `wavepart` = the wave number's bits already at their zb[] positions.
__device__ __forceinline__ unsigned zskip_index(unsigned lanebits, unsigned wavepart, uint64_t list, unsigned cnt)
{
    unsigned x = lanebits;
    for (unsigned k = 0; k < cnt; k++) x = (unsigned)insert_zero(x, (unsigned)(list >> (8u * k)) & 0xffu);
    return x | wavepart;
}
// does this wave's share of the tile (the elements whose zb[] bits spell its number) hold nothing but +0 ?
template <int TT>
__device__ __forceinline__ bool zskip_wave_is_zero(const amp_t *tile, const FusePass &P, unsigned wavepart)
{
    const unsigned lane = threadIdx.x & 63u;
    constexpr unsigned per = (1u << TT) >> 6;                   // elements per lane over the whole tile
    const unsigned share = per >> P.zskip;                        // ... of this wave's share
    uint64_t any = 0;
    for (unsigned k = 0; k < share; k++) {
        const amp_t v = tile[zskip_index(lane | (k << 6), wavepart, P.zlist, P.zskip)];
        any |= (uint64_t)__double_as_longlong(v.x) | (uint64_t)__double_as_longlong(v.y);
    }
    return __ballot(any != 0) == 0ULL;
}

template <int BLOCK, int TT, bool CAM = true, int TOL = 0>     // CAM = false: the pass holds no modular multiply (smaller kernel); TOL: 1 tolerance mode, 2 fast rounds only
__device__ __forceinline__ void fuse_apply_rounds(amp_t *tile, unsigned short *lut, const unsigned char *camtab,
                                                  const uint64_t *xm, const FusePass &P, const FuseOp *__restrict__ ops,
                                                  const FuseOp *ops_asm, uint64_t base, const amp_t *dg = nullptr, unsigned zrot = 0)
{
    static_assert((1u << TT) == 4u * BLOCK, "rounds form needs 4 amplitudes per thread");
    unsigned i = 0;
    // zskip: which share of the tile this wave takes rotates with the tile number (zrot) -- the populated shares are the same in
    // every tile, and a wave sits on one SIMD for good: without the rotation one SIMD would do all the work
    const unsigned zwave = ((threadIdx.x >> 6) + zrot) & ((BLOCK >> 6) - 1u);
    unsigned zpart = 0;
    for (unsigned j = 0; j < P.zskip; j++) zpart |= ((zwave >> j) & 1u) << P.zb[j];
    const bool idle = !CAM && P.zskip && zskip_wave_is_zero<TT>(tile, P, zpart);      // this wave holds nothing: it only keeps the barriers
    while (i < P.nops) {
        const uint32_t type = ops[i].type & 0xffu;
        if (TOL && type == FUSE_QROUND) {
            // tolerance mode, fast round  H(x) [D(x)] [H(y) [D(y)]]: straight-line, every table read issued up front
            const amp_t *gtab = dg + P.dg_cnt;                      // behind the per-tile E_out slots
            const unsigned rb0 = ops[i].a & 0xffu, rb1 = (ops[i].a >> 8) & 0xffu;
            const uint32_t sA = ops[i + 1].type, sB = ops[i + 1].a;
            if (!idle) {
            uint64_t zl; memcpy(&zl, &ops[i].c, sizeof zl);           // (zskip: the positions the lane number leaves out, sorted by the host)
            const unsigned p = P.zskip ? zskip_index(threadIdx.x & 63u, zpart, zl, P.zskip + 2u)
                                       : (unsigned)insert_zero(insert_zero(threadIdx.x, rb0), rb1);
            const unsigned e1 = p | (1u << rb0), e2 = p | (1u << rb1), e3 = e1 | (1u << rb1);
            if (sA & 1u) { if (sB & 1u) qround_run<true, true>(tile, p, e1, e2, e3, rb0, rb1, sA, sB, dg, gtab);
                           else         qround_run<true, false>(tile, p, e1, e2, e3, rb0, rb1, sA, sB, dg, gtab); }
            else         { if (sB & 1u) qround_run<false, true>(tile, p, e1, e2, e3, rb0, rb1, sA, sB, dg, gtab);
                           else         qround_run<false, false>(tile, p, e1, e2, e3, rb0, rb1, sA, sB, dg, gtab); }
            }
            __syncthreads();
            i += 2;
        } else if (TOL != 2 && type == FUSE_ROUND) {
            const unsigned rb0 = ops[i].a & 0xffu, rb1 = (ops[i].a >> 8) & 0xffu;
            const unsigned cnt = (unsigned)ops[i].mask;
            if (!idle) {
            uint64_t zl; memcpy(&zl, &ops[i].c, sizeof zl);           // (zskip: the positions the lane number leaves out, sorted by the host)
            const unsigned p = P.zskip ? zskip_index(threadIdx.x & 63u, zpart, zl, P.zskip + 2u)
                                       : (unsigned)insert_zero(insert_zero(threadIdx.x, rb0), rb1);
            const unsigned e1 = p | (1u << rb0), e2 = p | (1u << rb1), e3 = e1 | (1u << rb1);
            Quad q;
            { const amp_t v0 = tile[p], v1 = tile[e1], v2 = tile[e2], v3 = tile[e3];
              q.x0 = v0.x; q.y0 = v0.y; q.x1 = v1.x; q.y1 = v1.y; q.x2 = v2.x; q.y2 = v2.y; q.x3 = v3.x; q.y3 = v3.y; }
            // bit 16 of the header: the round contains an H.  It then canonicalises all amplitudes once at its end and
            // its phase runs skip their own canonical zeros (canon_bit clear).
            const bool has_h = (ops[i].a >> 16) & 1u;
            // items: the header's first dword says everything (one scalar load per item): type | code << 8 | gates << 16,
            // code as in fuse_round_item.  The records of a run's gates follow its header.
            // The walk reads the records through ops_asm, a second (non-restrict) kernel argument with the same value:
            // handing `ops` itself to an asm statement would count as a capture, after which the memory-clobbering
            // s_waitcnt statements of the pipeline could "modify" the records and every ops[] access in this function
            // would turn from a scalar load into a vector load.
            unsigned o = i + 1;
            const unsigned oend = i + cnt;
            const unsigned lane = threadIdx.x & 63u;
            // xm: the records' outside-tile masks staged in LDS (padded: a lane may look up to 64 entries past a run)
            const __attribute__((address_space(3))) uint64_t *xl = (const __attribute__((address_space(3))) uint64_t *)xm + o + 1 + lane;
            uint32_t xaddr = (uint32_t)(uintptr_t)xl;
            uint32_t t = ops[o].type;
            uint64_t m = *xl;
            do {        // a round has at least one item
                const unsigned rc = t >> 16;                             // 0 for an H: no live gates
                const uint64_t live = __builtin_amdgcn_ballot_w64((base & m) == m) & (rc >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << rc) - 1);
                uint32_t tn; uint64_t mn;
                fuse_round_item(q, ops_asm + o, live, p, t, xaddr, tn, mn);
                o += 1 + rc; t = tn; m = mn;
            } while (o <= oend);
            if (has_h) {
                q.x0 += 0.0; q.y0 += 0.0; q.x1 += 0.0; q.y1 += 0.0; q.x2 += 0.0; q.y2 += 0.0; q.x3 += 0.0; q.y3 += 0.0;
            }
            { amp_t v0, v1, v2, v3;
              v0.x = q.x0; v0.y = q.y0; v1.x = q.x1; v1.y = q.y1; v2.x = q.x2; v2.y = q.y2; v3.x = q.x3; v3.y = q.y3;
              tile[p] = v0; tile[e1] = v1; tile[e2] = v2; tile[e3] = v3; }
            }
            __syncthreads();
            i += 1 + cnt;
        } else if (CAM && type == FUSE_CAMRUN) {
            i += 1 + fuse_camrun_step<BLOCK, TT>(tile, lut, camtab, ops, i, base);
        } else if (CAM) {    // FUSE_CAMODC between rounds
            fuse_camodc_step<BLOCK, 4>(tile, lut, ops + i, base, 1u << TT);
            i++;
        } else {
            __builtin_unreachable();
        }
    }
}


template <int BLOCK, int TT, bool LDSDMA>   // TT = tile bits when known at compile time (loops unroll, loads batch); 0 = generic
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void k_fused(amp_t *__restrict__ amp, unsigned n, FusePass P,
                                                   const FuseOp *__restrict__ ops, uint64_t ntiles, const FuseOp *ops_asm)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char qcx_lds_raw[];
    amp_t *tile = reinterpret_cast<amp_t *>(qcx_lds_raw);
    const unsigned T = TT ? (unsigned)TT : P.T, c = P.c, nh = P.nh;
    const unsigned tsize = 1u << T;
    unsigned short *lut = reinterpret_cast<unsigned short *>(tile + tsize);  // behind the tile (host sizes the LDS)
    unsigned char *camtab = reinterpret_cast<unsigned char *>(lut) + P.cam_ctl_local[3];   // tables of folded multiply runs
    for (unsigned b = threadIdx.x; b < (unsigned)P.cam_ctl_local[1]; b += BLOCK)
        camtab[b] = reinterpret_cast<const unsigned char *>(ops + P.cam_ctl_local[2])[b];
    uint64_t *xm = P.xm_cnt ? reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(lut) + P.xm_off) : nullptr;
    for (unsigned b = threadIdx.x; b < P.xm_cnt + 66u && P.xm_cnt; b += BLOCK) xm[b] = b < P.xm_cnt ? ops[b].mask : 0;    // + padding
    __syncthreads();
    constexpr unsigned EPT = TT ? ((1u << TT) + BLOCK - 1) / BLOCK : 16;      // elements per thread (<= 16)
    const unsigned ept = TT ? EPT : (tsize + BLOCK - 1) / BLOCK;
    (void)c; (void)nh;
    // global offset of a tile-local element index: linear in its bits, so split thread part / k part (this kernel works in
    // place on the identity layout: the output tables of FusePass equal the input ones)
    auto scatter = [&](unsigned e) -> uint64_t { return fuse_spread(e, P.in_pos, T); };
    const uint64_t off_t = scatter(threadIdx.x);
    uint64_t off_k[EPT];
#pragma unroll
    for (unsigned k = 0; k < EPT; k++) off_k[k] = scatter(k * BLOCK);

    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = fuse_deposit(t, P.seg_in, P.nseg_in);
        amp_t *g = amp + (base | off_t);

        if constexpr (TT != 0 && LDSDMA) {
            // LDS-DMA: every wave instruction moves 64 x 16 B straight from HBM into 1 KiB of the tile
            // (lane l lands at base + 16 l); no staging registers, all loads of the tile in flight at once
            const unsigned wbase = (threadIdx.x >> 6) * 64;
#pragma unroll
            for (unsigned k = 0; k < EPT; k++)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + off_k[k]),
                                                 (__attribute__((address_space(3))) void *)(tile + k * BLOCK + wbase), 16, 0, 2);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {   // all loads of the tile in flight before the first LDS write
            amp_t v[EPT];
#pragma unroll
            for (unsigned k = 0; k < EPT; k++)
                if (k < ept && k * BLOCK + threadIdx.x < tsize) v[k] = __builtin_nontemporal_load(g + off_k[k]);
#pragma unroll
            for (unsigned k = 0; k < EPT; k++)
                if (k < ept && k * BLOCK + threadIdx.x < tsize) tile[k * BLOCK + threadIdx.x] = v[k];
        }
        __syncthreads();

        if constexpr (TT != 0 && (1u << TT) == 4u * BLOCK) {
            if (P.cam_ctl_local[0]) fuse_apply_rounds<BLOCK, TT>(tile, lut, camtab, xm, P, ops, ops_asm, base);
            else fuse_apply_ops<BLOCK, TT, EPT>(tile, lut, P, ops, base, off_t, off_k, tsize, ept);
        } else {
            fuse_apply_ops<BLOCK, TT, EPT>(tile, lut, P, ops, base, off_t, off_k, tsize, ept);
        }

        {
            amp_t v[EPT];
#pragma unroll
            for (unsigned k = 0; k < EPT; k++)
                if (k < ept && k * BLOCK + threadIdx.x < tsize) v[k] = tile[k * BLOCK + threadIdx.x];
#pragma unroll
            for (unsigned k = 0; k < EPT; k++)
                if (k < ept && k * BLOCK + threadIdx.x < tsize) __builtin_nontemporal_store(v[k], g + off_k[k]);
        }
        __syncthreads();
    }
}

// The ROUNDS form on its own: the kernel the scheduler launches for every pass in rounds form (4 amplitudes per
// thread: BLOCK = 2^TT / 4).  One tile per workgroup at a time, LDS-DMA fill, a grid of a few workgroups per CU
// slot that walk the tiles (the table fill below is paid once per workgroup, not once per tile).  Load / process /
// store phases of the resident workgroups overlap each other; measured, that beats the double-buffered pipeline
// inside one workgroup (the round-1 pipelined form, removed) as soon as enough workgroups are resident, so this kernel carries nothing but
// the rounds interpreter and is held to OCC waves per SIMD.
template <int BLOCK, int TT, int OCC, bool CAM, int TOL = 0, bool GEN = false>      // GEN: the tiles are generated, not read (GenFront)
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(OCC))) void k_fused_rounds(
    const amp_t *amp, amp_t *amp_out, unsigned n, FusePass P, const FuseOp *__restrict__ ops, uint64_t ntiles, const FuseOp *ops_asm)
{
    static_assert((1u << TT) == 4u * BLOCK, "rounds form: 4 amplitudes per thread");
    extern __shared__ __attribute__((aligned(16))) unsigned char qcx_lds_raw[];
    amp_t *tile = reinterpret_cast<amp_t *>(qcx_lds_raw);
    constexpr unsigned tsize = 1u << TT;
    unsigned short *lut = reinterpret_cast<unsigned short *>(tile + tsize);
    unsigned char *camtab = reinterpret_cast<unsigned char *>(lut) + P.cam_ctl_local[3];
    for (unsigned b = threadIdx.x; b < (unsigned)P.cam_ctl_local[1]; b += BLOCK)
        camtab[b] = reinterpret_cast<const unsigned char *>(ops + P.cam_ctl_local[2])[b];
    uint64_t *xm = reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(lut) + P.xm_off);
    if constexpr (TOL != 2)
        for (unsigned b = threadIdx.x; b < P.xm_cnt + 66u; b += BLOCK) xm[b] = b < P.xm_cnt ? ops[b].mask : 0;    // + padding
    // tolerance mode: [E_out slot per diagonal][G tables, 48 entries per diagonal] in LDS; the tables are staged once
    amp_t *dg = reinterpret_cast<amp_t *>(reinterpret_cast<unsigned char *>(lut) + P.dg_lds_off);
    const amp_t *dg_area = reinterpret_cast<const amp_t *>(ops + P.dg_rec_off);             // global: DiagInfo[], G tables, field tables
    if constexpr (TOL)
        for (unsigned b = threadIdx.x; b < P.dg_cnt * 48u; b += BLOCK) dg[P.dg_cnt + b] = dg_area[3u * P.dg_cnt + b];
    __syncthreads();
    const uint64_t off_t = fuse_spread(threadIdx.x, P.in_pos, TT);
    uint64_t off_k[4], st_k[4];
    unsigned ld_k[4];
#pragma unroll
    for (unsigned k = 0; k < 4; k++) {
        off_k[k] = fuse_spread(k * BLOCK, P.in_pos, TT);
        st_k[k] = fuse_spread(k * BLOCK, P.st_pos, TT);
        ld_k[k] = (unsigned)fuse_spread(k * BLOCK, P.st_loc, TT);
    }
    const uint64_t st_t = fuse_spread(threadIdx.x, P.st_pos, TT);
    const unsigned ld_t = (unsigned)fuse_spread(threadIdx.x, P.st_loc, TT);
    const unsigned wbase = (threadIdx.x >> 6) * 64;
    // gen: the tiles are generated (the circuit front on a basis state that was never written), not read
    const GenFront *GF = reinterpret_cast<const GenFront *>(ops + P.gen_rec_off);
    unsigned short *gen_phot = reinterpret_cast<unsigned short *>(reinterpret_cast<unsigned char *>(lut) + P.gen_lds_off);
    unsigned short *gen_res = gen_phot + 1024;
    uint32_t packT = 0, packK[4] = {0, 0, 0, 0};
    if constexpr (GEN) {
        gen_setup<BLOCK>(GF, gen_phot);
        packT = gen_pack(threadIdx.x, GF, TT);
#pragma unroll
        for (unsigned k = 0; k < 4; k++) packK[k] = gen_pack(k * BLOCK, GF, TT);
        __syncthreads();
    }
    const unsigned slog = (P.dbg >> 12) & 15u;
    for (uint64_t b0 = blockIdx.x; b0 < ntiles; b0 += gridDim.x) {
        const uint64_t t = fuse_stream_tile(b0, n - TT, slog, (P.dbg >> 16) & 31u);       // (round 3's fuse_swz, the same idea for this kernel alone, is gone)
        const uint64_t base_in = fuse_deposit(t, P.seg_in, P.nseg_in);
        uint64_t base = base_in, base_out = base_in;               // logical base (gate records), output base
        if (P.chained) { base = fuse_deposit(t, P.seg_lg, P.nseg_lg); base_out = fuse_deposit(t, P.seg_out, P.nseg_out); }
        const amp_t *g = amp + (base_in | off_t);
        amp_t *go = amp_out + (base_out | st_t);
        if constexpr (GEN) gen_tile<BLOCK, 4>(GF, tile, gen_phot, gen_res, base, packT, packK);
        else if (!(P.dbg & 4u)) {
#pragma unroll
            for (unsigned k = 0; k < 4; k++)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + off_k[k]),
                                                 (__attribute__((address_space(3))) void *)(tile + k * BLOCK + wbase), 16, 0, 2);
        }
        if constexpr (TOL) {
            // E_out of this tile for every diagonal of the pass: one thread each, while the tile fill is in flight
            if (threadIdx.x < P.dg_cnt) {
                const DiagInfo *info = reinterpret_cast<const DiagInfo *>(dg_area) + threadIdx.x;
                const uint32_t present = info->present;
                amp_t E; E.x = info->kc; E.y = info->ks;
#pragma unroll
                for (unsigned f = 0; f < 5; f++)
                    if ((present >> f) & 1u) cmul_tol(E, dg_area[info->field_off[f] + (unsigned)((base >> (8u * f)) & 255u)]);
                dg[threadIdx.x] = E;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (!(P.dbg & 1u)) fuse_apply_rounds<BLOCK, TT, CAM, TOL>(tile, lut, camtab, xm, P, ops, ops_asm, base, dg, (unsigned)t);
        amp_t v[4];
#pragma unroll
        for (unsigned k = 0; k < 4; k++) v[k] = tile[ld_k[k] | ld_t];          // (store order: ascending OUTPUT positions)
        if (!(P.dbg & 2u)) {
#pragma unroll
            for (unsigned k = 0; k < 4; k++) __builtin_nontemporal_store(v[k], go + st_k[k]);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// K6g  the generated first pass of a circuit by COLUMNS (FusePass::gen = 2; bit-exact).  Behind a circuit front only a few of
// the 2^M low index values are populated -- the residues of the multiply ladder's orbit (C = 21, a = 2: six of 32) -- and no
// gate of an inverse QFT touches the M register, so an amplitude's low bits never change: the tile of 2^12 amplitudes =
// 16 values of the four lowest M-register bits x 2^8 combinations of eight hot bits falls into 16 independent COLUMNS of
// which at most a handful hold anything but +0.  The workgroup (256 threads = the 2^8 hot combinations) generates the tile
// as GenFront says, keeps ONLY the populated columns in LDS (maxcols of them, host-computed bound from the orbit; 257
// elements apart so that the store's column-major reads spread over the banks), and each wave takes whole columns through
// all rounds of the pass on its own: a column is 64 lanes x 4 registers, so there is no barrier between rounds and no wave
// without work -- the k_fused_rounds form of this pass spends half of its waves on zeros (zskip finds a quarter or three
// quarters of a 2^10 tile empty) or, on 2^12 tiles, leaves 13 of 16 waves of a 64-KiB workgroup idle.  Empty columns are
// stored as +0 straight from registers.  Same records, same walk (fuse_round_item), same bits.
// ---------------------------------------------------------------------------
#define QCX_COL_STRIDE 257u
// A workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for the wave's outstanding GLOBAL stores
// (s_waitcnt vmcnt(0) in front of s_barrier): inside k_gen_cols' tile loop that made every wave sit out the round trip of the
// tile it had just stored before it could generate the next one -- and since all workgroups of a CU run in step, the chip
// alternated between computing and storing.  The loop has no vector load from global memory (records: scalar loads, masks and
// tables: LDS), so nothing in it needs the stores to have landed; they drain while the next tile is generated and walked.
#define QCX_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
// x mod C with the host's Cinv = floor(2^32 / C): the quotient estimate is at most one short
__device__ __forceinline__ unsigned gen_mod(unsigned x, unsigned C, unsigned Cinv)
{
    unsigned r = x - __umulhi(x, Cinv) * C;
    return r >= C ? r - C : r;
}
// gen = 2: on the register itself -- tile = its four lowest M-register bits x 8 hot bits, columns = the values of those four
//          bits, the populated ones found per tile (a tile whose other M-register bits, outside the tile, do not match a
//          residue holds nothing there);
// gen = 3: on the VIRTUAL register of a compact chain (qcx_fuse.inc.h) -- index = [L-register bits][column], cb column bits,
//          column j = the amplitudes whose M register reads GenFront::orbit[j]: every column is kept, the store writes the
//          compact layout (the real index of a tile's base is its L part shifted up by M).
// Launched with 64 * W threads, W = 4 ... 8 (fuse_cols_waves; 4 by default): the first 256 threads generate and store the tile,
// further waves only walk columns.
template <int OCC, bool TOL = false>     // TOL: the pass holds merged diagonals (tolerance mode): fast rounds run as in k_fused_rounds<.., TOL>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(OCC))) void k_gen_cols(
    amp_t *__restrict__ amp_out, unsigned n, FusePass P, const FuseOp *__restrict__ ops, uint64_t ntiles, const FuseOp *ops_asm)
{
    constexpr unsigned BLOCK = 256;
    const unsigned nthreads = blockDim.x, nwaves = blockDim.x >> 6;
    const bool worker = threadIdx.x < BLOCK;                                      // takes part in generating and storing
    extern __shared__ __attribute__((aligned(16))) unsigned char qcx_lds_raw[];
    const unsigned maxcols = P.zpad;
    amp_t *cols = reinterpret_cast<amp_t *>(qcx_lds_raw);                         // [maxcols][QCX_COL_STRIDE]
    unsigned char *behind = reinterpret_cast<unsigned char *>(cols + maxcols * QCX_COL_STRIDE);
    uint64_t *xm = reinterpret_cast<uint64_t *>(behind + P.xm_off);
    for (unsigned b = threadIdx.x; b < P.xm_cnt + 66u; b += nthreads) xm[b] = b < P.xm_cnt ? ops[b].mask : 0;    // + padding
    __shared__ unsigned s_mask;
    // tolerance mode: [E_out slot per diagonal][G tables, 48 entries per diagonal] in LDS; the tables are staged once
    amp_t *dg = reinterpret_cast<amp_t *>(behind + P.dg_lds_off);
    const amp_t *dg_area = reinterpret_cast<const amp_t *>(ops + P.dg_rec_off);
    if constexpr (TOL)
        for (unsigned b = threadIdx.x; b < P.dg_cnt * 48u; b += nthreads) dg[P.dg_cnt + b] = dg_area[3u * P.dg_cnt + b];
    const GenFront *GF = reinterpret_cast<const GenFront *>(ops + P.gen_rec_off);
    const bool compact = P.gen == 3;
    const unsigned cb = compact ? GF->cb : 4u, TT = cb + 8u, cmask = (1u << cb) - 1u;
    // this thread IS hot combination h = threadIdx.x (tile-local bits cb .. cb + 7; slot h of the generated fill)
    const unsigned h = threadIdx.x & 255u, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned phot = GF->f0;                                                       // residue factor of the tile-local controls, times f0
    if (!worker || (h & GF->sfm) != GF->sbv) phot = 0xffffu;
    else if (GF->C)
        for (unsigned g = 0; g < GF->ncam; g++)
            if (GF->camloc[g] != 0xff && ((h >> GF->camloc[g]) & 1u)) phot = gen_mod(phot * GF->camA[g], GF->C, GF->Cinv);
    const uint32_t parH = compact ? ((uint32_t)__builtin_popcount(h & GF->sgn_slots) & 1u) : ((gen_pack(h << 4, GF, TT) >> 24) & 1u);
    const uint64_t st_t = fuse_spread(threadIdx.x, P.st_pos, TT);
    const unsigned ld_t = (unsigned)fuse_spread(threadIdx.x, P.st_loc, TT);
    // store order: element k * 256 + thread of the OUTPUT order; the bits of k spread linearly (uniform values)
    unsigned bl[4]; uint64_t bp[4];
#pragma unroll
    for (unsigned b = 0; b < 4; b++) { bl[b] = (unsigned)fuse_spread(256u << b, P.st_loc, TT); bp[b] = fuse_spread(256u << b, P.st_pos, TT); }
    if (threadIdx.x == 0) s_mask = 0;
    // the front's constants, read ONCE: amp_out may alias the record buffer as far as the compiler knows, so every GF-> access
    // inside the tile loop was a fresh scalar load -- some twenty per tile, half of them in a dependent chain (the orbit search, the
    // factor tables): 0.73 ms of the pass at n = 30 was this latency (generation alone, gates and stores skipped)
    const uint64_t gf_fixed_out = GF->fixed_out, gf_fixed_val = GF->basis & GF->fixed_out, gf_sign_out = GF->sign_out;
    const double gf_v = GF->v;
    const unsigned gf_C = GF->C, gf_Cinv = GF->Cinv, gf_present = GF->present, gf_M = GF->M, gf_lowout = GF->lowout_mask, gf_ncols = GF->ncols;
    // compact form: column of a residue, tabulated once per workgroup (residues < C <= 4096; 0xff: not on the orbit)
    unsigned char *col_of = reinterpret_cast<unsigned char *>(behind + P.gen_lds_off);
    if (compact) {
        for (unsigned f = threadIdx.x; f < (gf_C ? gf_C : (1u << gf_M)); f += nthreads) {
            unsigned char c = 0xff;
            for (unsigned jj = 0; jj < gf_ncols; jj++) if (GF->orbit[jj] == f) c = (unsigned char)jj;
            col_of[f] = c;
        }
    }
    __syncthreads();
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base_in = fuse_deposit(t, P.seg_in, P.nseg_in);
        uint64_t base = base_in, base_out = base_in;
        if (P.chained) { base = fuse_deposit(t, P.seg_lg, P.nseg_lg); base_out = fuse_deposit(t, P.seg_out, P.nseg_out); }
        amp_t *go = amp_out + (base_out | st_t);
        const uint64_t rbase = compact ? (base >> cb) << gf_M : base;            // the tile's base as an index of the REAL register
        // ---- generate: this thread's one candidate amplitude (hot combination h): its residue, column and sign ----------
        unsigned f = 0xffffu;
        if ((rbase & gf_fixed_out) == gf_fixed_val && phot != 0xffffu) {
            f = phot;
            if (gf_C) {
                unsigned pt = 1;                                                  // controls outside the tile: one factor per tile
#pragma unroll
                for (unsigned k = 0; k < 5; k++)
                    if ((gf_present >> k) & 1u) pt = gen_mod(pt * (unsigned)GF->tabP[k][(unsigned)((rbase >> (8u * k)) & 255u)], gf_C, gf_Cinv);
                f = gen_mod(f * pt, gf_C, gf_Cinv);
            }
            if (!compact && (f & gf_lowout) != ((uint32_t)base & gf_lowout)) f = 0xffffu;   // its low bits outside the tile belong to another tile
        }
        if constexpr (TOL) {
            // E_out of this tile for every diagonal of the pass: one thread each (read by the rounds, behind the barriers below)
            if (threadIdx.x < P.dg_cnt) {
                const DiagInfo *info = reinterpret_cast<const DiagInfo *>(dg_area) + threadIdx.x;
                const uint32_t present = info->present;
                amp_t E; E.x = info->kc; E.y = info->ks;
#pragma unroll
                for (unsigned k = 0; k < 5; k++)
                    if ((present >> k) & 1u) cmul_tol(E, dg_area[info->field_off[k] + (unsigned)((base >> (8u * k)) & 255u)]);
                dg[threadIdx.x] = E;
            }
        }
        unsigned mycol = f & 15u;
        if (compact) {                                                            // column = the residue's place in the orbit
            mycol = f != 0xffffu ? (unsigned)col_of[f] : 0xffu;
            if (mycol == 0xffu) f = 0xffffu;                                      // (cannot happen: the orbit holds every reachable residue)
        } else if (f != 0xffffu) atomicOr(&s_mask, 1u << mycol);
        QCX_LDS_BARRIER();
        const unsigned mask = compact ? (1u << gf_ncols) - 1u : s_mask;
        const unsigned ncol = (unsigned)__builtin_popcount(mask);
        if (worker) for (unsigned s = 0; s < ncol; s++) { amp_t z; z.x = 0.0; z.y = 0.0; cols[s * QCX_COL_STRIDE + h] = z; }
        if (f != 0xffffu) {
            const uint32_t par = (parH ^ (uint32_t)__builtin_popcountll(rbase & gf_sign_out)) & 1u;
            amp_t a; a.x = par ? -gf_v : gf_v; a.y = 0.0;
            cols[(unsigned)__builtin_popcount(mask & ((1u << mycol) - 1u)) * QCX_COL_STRIDE + h] = a;
        }
        QCX_LDS_BARRIER();
        // ---- rounds: every wave takes whole columns through the pass on its own --------------------------------------
        // (which columns a wave takes rotates with the tile number: six columns over four waves are 2 + 2 + 1 + 1, a wave sits on one
        //  SIMD for good, and with a fixed assignment SIMDs 0 and 1 of every CU would carry twice the work of SIMDs 2 and 3)
        if (!(P.dbg & 1u))
        for (unsigned s = (wave + (unsigned)t + (unsigned)(t >> 2)) % nwaves; s < ncol; s += nwaves) {
            unsigned cpat = 0;                                                    // the column's low-bit value: the s-th set bit of mask
            { unsigned m = mask; for (unsigned k = 0; k < s; k++) m &= m - 1u; cpat = (unsigned)__builtin_ctz(m); }
            amp_t *col = cols + s * QCX_COL_STRIDE;
            unsigned i = 0;
            while (i < P.nops) {
                const unsigned rb0 = (ops[i].a & 0xffu) - cb, rb1 = ((ops[i].a >> 8) & 0xffu) - cb;     // (hot bits; the host checks)
                const unsigned cnt = (unsigned)ops[i].mask;
                const unsigned hh = (unsigned)insert_zero(insert_zero(lane, rb0), rb1);
                const unsigned p = (hh << cb) | cpat;                                     // logical tile-local index (the walk tests its bits)
                const unsigned l0 = hh, l1 = hh | (1u << rb0), l2 = hh | (1u << rb1), l3 = l1 | l2;
                if (TOL && (ops[i].type & 0xffu) == FUSE_QROUND) {
                    const amp_t *gtab = dg + P.dg_cnt;
                    const uint32_t sA = ops[i + 1].type, sB = ops[i + 1].a;
                    if (sA & 1u) { if (sB & 1u) qround_run_col<true, true>(col, l0, l1, l2, l3, p, rb0 + cb, rb1 + cb, sA, sB, dg, gtab);
                                   else         qround_run_col<true, false>(col, l0, l1, l2, l3, p, rb0 + cb, rb1 + cb, sA, sB, dg, gtab); }
                    else         { if (sB & 1u) qround_run_col<false, true>(col, l0, l1, l2, l3, p, rb0 + cb, rb1 + cb, sA, sB, dg, gtab);
                                   else         qround_run_col<false, false>(col, l0, l1, l2, l3, p, rb0 + cb, rb1 + cb, sA, sB, dg, gtab); }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_wave_barrier();
                    i += 2;
                    continue;
                }
                Quad q;
                { const amp_t v0 = col[l0], v1 = col[l1], v2 = col[l2], v3 = col[l3];
                  q.x0 = v0.x; q.y0 = v0.y; q.x1 = v1.x; q.y1 = v1.y; q.x2 = v2.x; q.y2 = v2.y; q.x3 = v3.x; q.y3 = v3.y; }
                const bool has_h = (ops[i].a >> 16) & 1u;
                unsigned o = i + 1;
                const unsigned oend = i + cnt;
                const __attribute__((address_space(3))) uint64_t *xl = (const __attribute__((address_space(3))) uint64_t *)xm + o + 1 + lane;
                uint32_t xaddr = (uint32_t)(uintptr_t)xl;
                uint32_t ty = ops[o].type;
                uint64_t m = *xl;
                do {
                    const unsigned rc = ty >> 16;
                    const uint64_t live = __builtin_amdgcn_ballot_w64((base & m) == m) & (rc >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << rc) - 1);
                    uint32_t tn; uint64_t mn;
                    fuse_round_item(q, ops_asm + o, live, p, ty, xaddr, tn, mn);
                    o += 1 + rc; ty = tn; m = mn;
                } while (o <= oend);
                if (has_h) {
                    q.x0 += 0.0; q.y0 += 0.0; q.x1 += 0.0; q.y1 += 0.0; q.x2 += 0.0; q.y2 += 0.0; q.x3 += 0.0; q.y3 += 0.0;
                }
                { amp_t v0, v1, v2, v3;
                  v0.x = q.x0; v0.y = q.y0; v1.x = q.x1; v1.y = q.y1; v2.x = q.x2; v2.y = q.y2; v3.x = q.x3; v3.y = q.y3;
                  col[l0] = v0; col[l1] = v1; col[l2] = v2; col[l3] = v3; }
                // (the column is this wave's own: its LDS accesses are served in order, no workgroup barrier between rounds)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
                i += 1 + cnt;
            }
        }
        QCX_LDS_BARRIER();
        if (threadIdx.x == 0) s_mask = 0;                                         // (read by everyone before the barrier above)
        // ---- store the whole tile: populated columns from LDS, the others as +0 ------------------------------------------
        if (worker && !(P.dbg & 2u)) {
            const unsigned nk = 1u << cb;
#pragma unroll
            for (unsigned k = 0; k < 16; k++) {
                if (k >= nk) break;
                unsigned elk = 0; uint64_t offk = 0;
#pragma unroll
                for (unsigned b = 0; b < 4; b++) if ((k >> b) & 1u) { elk |= bl[b]; offk |= bp[b]; }
                const unsigned el = elk | ld_t;                                   // tile-local element, in store order
                const unsigned c = el & cmask, eh = el >> cb;
                amp_t v; v.x = 0.0; v.y = 0.0;
                if ((mask >> c) & 1u) v = cols[(unsigned)__builtin_popcount(mask & ((1u << c) - 1u)) * QCX_COL_STRIDE + eh];
                __builtin_nontemporal_store(v, go + offk);
            }
        }
        QCX_LDS_BARRIER();
    }
}

// the end of a compact chain: the real register from its compact form.  real[(l << M) | f] = compact[(l << cb) | j] where
// f = orbit[j], and +0 for every other f; the whole register is written (16 * 2^n bytes).  A workgroup takes 64 blocks at a
// time: their compact rows (64 * 2^cb amplitudes, contiguous) are staged in LDS with coalesced loads, then the 64 * 2^M real
// amplitudes leave as coalesced nontemporal stores (a per-amplitude gather of the compact form kept a dependent load in front
// of every store: 8.0 ms at n = 30 against 3 ms for the bytes).  direct: no stage -- a thread loads the (few) compact sources of
// its next 8 real amplitudes first, then stores the 8: 3.76 against 4.02 ms (the default).
struct ExpandParams { unsigned M, cb, ncols; uint16_t orbit[16]; };
__global__ __launch_bounds__(256) void k_expand_compact(const amp_t *__restrict__ compact, amp_t *__restrict__ real, uint64_t nchunks, ExpandParams E, int direct)
{
    __shared__ __attribute__((aligned(16))) amp_t stage[64 << 4];
    __shared__ unsigned char lut[1 << 12];
    const unsigned M = E.M, cb = E.cb, lowmask = (1u << M) - 1u;
    for (unsigned f = threadIdx.x; f <= lowmask; f += 256) {
        unsigned char j = 0xff;
        for (unsigned k = 0; k < E.ncols; k++) if (E.orbit[k] == f) j = (unsigned char)k;
        lut[f] = j;
    }
    __syncthreads();
    if (direct) {
        // variant without the LDS stage: 8 real amplitudes per thread, their (few) compact sources loaded first, then 8 stores
        for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
            const amp_t *from = compact + ((chunk * 64) << cb);
            amp_t *to = real + ((chunk * 64) << M);
            for (unsigned e0 = threadIdx.x; e0 < (64u << M); e0 += 256u * 8u) {
                amp_t v[8];
#pragma unroll
                for (unsigned k = 0; k < 8; k++) {
                    const unsigned e = e0 + k * 256u;
                    const unsigned j = e < (64u << M) ? lut[e & lowmask] : 0xffu;
                    v[k].x = 0.0; v[k].y = 0.0;
                    if (j != 0xffu) v[k] = from[((e >> M) << cb) | j];
                }
#pragma unroll
                for (unsigned k = 0; k < 8; k++) if (e0 + k * 256u < (64u << M)) __builtin_nontemporal_store(v[k], to + e0 + k * 256u);
            }
        }
        return;
    }
    for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const amp_t *from = compact + ((chunk * 64) << cb);
        for (unsigned e = threadIdx.x; e < (64u << cb); e += 256) stage[e] = __builtin_nontemporal_load(from + e);
        __syncthreads();
        amp_t *to = real + ((chunk * 64) << M);
        for (unsigned e = threadIdx.x; e < (64u << M); e += 256) {
            const unsigned j = lut[e & lowmask];
            amp_t v; v.x = 0.0; v.y = 0.0;
            if (j != 0xffu) v = stage[((e >> M) << cb) | j];
            __builtin_nontemporal_store(v, to + e);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// K6t-8  tolerance mode, RADIX-8 fast rounds on 2^12-amplitude tiles: a thread keeps the 8 amplitudes that differ in THREE
// register bits, a round is up to three steps  H(x) [D(x)]  -- three Hadamards and their merged diagonals per LDS round trip
// and per barrier instead of two, with 512-thread workgroups (8 waves) on a tile that holds 8 hot bits: the n = 28 inverse
// QFT in 3 passes instead of 4.  Passes whose rounds are ALL of that shape and that hold no modular multiply take this
// kernel; everything else takes k_fused_rounds.
// Records: FUSE_QROUND3  a = rb0 | rb1 << 8 | rb2 << 16 | steps << 24, mask = 1 (one record follows), then one record with
// the step words in type, a and the low half of mask.  Step word: bits 0-1 = which register bit (0..2), bit 2 = a diagonal
// follows the H, bits 8-15 its slot, bits 16-18 its groups, bit 19 / 20 = the lower / higher of the OTHER two register
// bits is one of its targets.
// ---------------------------------------------------------------------------
enum : uint32_t { FUSE_QROUND3 = 8 };

// Hadamard butterfly WITHOUT its 1/sqrt(2): the radix-8 passes multiply every amplitude by (1/sqrt 2)^(Hadamards of the pass)
// once, when the tile is stored (every amplitude of a tile takes part in every Hadamard of the pass)
__device__ __forceinline__ void h_butterfly_unscaled(amp_t &a, amp_t &b)
{
    const double ar = a.x, ai = a.y;
    a.x = ar + b.x;  a.y = ai + b.y;
    b.x = ar - b.x;  b.y = ai - b.y;
}

// the exact Hadamard butterfly without its trailing "+ 0.0" (the pass canonicalises once, when the tile is stored)
__device__ __forceinline__ void h_butterfly_noz(amp_t &a, amp_t &b)
{
    const double s = QCX_SQRT1_2;
    const double t0r = s * a.x, t0i = s * a.y, t1r = s * b.x, t1i = s * b.y;
    a.x = t0r + t1r;  a.y = t0i + t1i;
    b.x = t0r - t1r;  b.y = t0i - t1i;
}

template <int R, bool EXACT>        // step on register bit R of an 8-amplitude register file (index bit j of v[] = register bit j)
__device__ __forceinline__ void q3_step(uint32_t s, unsigned p, unsigned rbo1, unsigned rbo2, amp_t (&v)[8], const amp_t *dg, const amp_t *gtab)
{
    constexpr int O1 = (R == 0) ? 1 : 0, O2 = (R == 2) ? 1 : 2;          // the other two register bits, ascending
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            if constexpr (EXACT) h_butterfly_noz(v[(a << O1) | (b << O2)], v[(1 << R) | (a << O1) | (b << O2)]);
            else h_butterfly_unscaled(v[(a << O1) | (b << O2)], v[(1 << R) | (a << O1) | (b << O2)]);
        }
    if constexpr (EXACT) return;
    if (s & 4u) {
        const unsigned slot = (s >> 8) & 0xffu;
        const amp_t *G = gtab + slot * 48u;
        amp_t F = dg[slot];
        if (s & (1u << 16)) cmul_tol(F, G[p & 15u]);
        if (s & (1u << 17)) cmul_tol(F, G[16u + ((p >> 4) & 15u)]);
        if (s & (1u << 18)) cmul_tol(F, G[32u + (p >> 8)]);
        amp_t F1 = F, F2 = F;
        if (s & (1u << 19)) cmul_tol(F1, G[16u * (rbo1 >> 2) + (1u << (rbo1 & 3u))]);
        if (s & (1u << 20)) { const amp_t w2 = G[16u * (rbo2 >> 2) + (1u << (rbo2 & 3u))]; cmul_tol(F2, w2); amp_t F3 = F1; cmul_tol(F3, w2);
                              cmul_tol(v[(1 << R) | (1 << O1) | (1 << O2)], F3); }
        else cmul_tol(v[(1 << R) | (1 << O1) | (1 << O2)], F1);
        cmul_tol(v[1 << R], F);
        cmul_tol(v[(1 << R) | (1 << O1)], F1);
        cmul_tol(v[(1 << R) | (1 << O2)], F2);
    }
}

template <int RA, int RB, int RC, bool EXACT>
__device__ __forceinline__ void q3_run(amp_t *tile, unsigned p, const unsigned (&rb)[3], unsigned nsteps, uint32_t sA, uint32_t sB, uint32_t sC,
                                       const amp_t *dg, const amp_t *gtab)
{
    amp_t v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = tile[p | ((j & 1u) << rb[0]) | (((j >> 1) & 1u) << rb[1]) | ((unsigned)(j >> 2) << rb[2])];
    q3_step<RA, EXACT>(sA, p, rb[RA == 0 ? 1 : 0], rb[RA == 2 ? 1 : 2], v, dg, gtab);
    __builtin_amdgcn_sched_barrier(0);
    if (nsteps > 1) q3_step<RB, EXACT>(sB, p, rb[RB == 0 ? 1 : 0], rb[RB == 2 ? 1 : 2], v, dg, gtab);
    __builtin_amdgcn_sched_barrier(0);
    if (nsteps > 2) q3_step<RC, EXACT>(sC, p, rb[RC == 0 ? 1 : 0], rb[RC == 2 ? 1 : 2], v, dg, gtab);
#pragma unroll
    for (int j = 0; j < 8; j++) tile[p | ((j & 1u) << rb[0]) | (((j >> 1) & 1u) << rb[1]) | ((unsigned)(j >> 2) << rb[2])] = v[j];
}

// EXACT = true: the same radix-8 structure for passes of nothing but Hadamards in the BIT-EXACT modes (the fused Hadamard
// sweep): exact butterflies (separate roundings, no FMA), canonical zeros once at the store; no tables, no diagonals.
template <int BLOCK, int TT, int OCC, bool EXACT = false, bool GEN = false>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(OCC))) void k_fused_q3(
    const amp_t *amp, amp_t *amp_out, unsigned n, FusePass P, const FuseOp *__restrict__ ops, uint64_t ntiles)
{
    static_assert((1u << TT) == 8u * BLOCK, "radix-8 rounds: 8 amplitudes per thread");
    extern __shared__ __attribute__((aligned(16))) unsigned char qcx_lds_raw[];
    amp_t *tile = reinterpret_cast<amp_t *>(qcx_lds_raw);
    constexpr unsigned tsize = 1u << TT;
    amp_t *dg = reinterpret_cast<amp_t *>(reinterpret_cast<unsigned char *>(tile + tsize) + P.dg_lds_off);
    const amp_t *dg_area = reinterpret_cast<const amp_t *>(ops + P.dg_rec_off);
    bool staged = EXACT;                 // (the diagonals' G tables are staged once per workgroup, behind the first tile's fill: see below)
    const amp_t *gtab = dg + P.dg_cnt;
    const uint64_t off_t = fuse_spread(threadIdx.x, P.in_pos, TT);
    uint64_t off_k[8], st_k[8];
    unsigned ld_k[8];
#pragma unroll
    for (unsigned k = 0; k < 8; k++) {
        off_k[k] = fuse_spread(k * BLOCK, P.in_pos, TT);
        st_k[k] = fuse_spread(k * BLOCK, P.st_pos, TT);
        ld_k[k] = (unsigned)fuse_spread(k * BLOCK, P.st_loc, TT);
    }
    const uint64_t st_t = fuse_spread(threadIdx.x, P.st_pos, TT);
    const unsigned ld_t = (unsigned)fuse_spread(threadIdx.x, P.st_loc, TT);
    const unsigned wbase = (threadIdx.x >> 6) * 64;
    // gen: the tiles are generated (the circuit front on a basis state that was never written), not read
    const GenFront *GF = reinterpret_cast<const GenFront *>(ops + P.gen_rec_off);
    unsigned short *gen_phot = reinterpret_cast<unsigned short *>(reinterpret_cast<unsigned char *>(tile + tsize) + P.gen_lds_off);
    unsigned short *gen_res = gen_phot + 512;
    uint32_t packT = 0, packK[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (GEN) {
        gen_setup<BLOCK>(GF, gen_phot);
        packT = gen_pack(threadIdx.x, GF, TT);
#pragma unroll
        for (unsigned k = 0; k < 8; k++) packK[k] = gen_pack(k * BLOCK, GF, TT);
        __syncthreads();
    }
    const unsigned slog = (P.dbg >> 12) & 15u;
    for (uint64_t b0 = blockIdx.x; b0 < ntiles; b0 += gridDim.x) {
        const uint64_t t = fuse_stream_tile(b0, n - TT, slog, (P.dbg >> 16) & 31u);
        const uint64_t base_in = fuse_deposit(t, P.seg_in, P.nseg_in);
        uint64_t base = base_in, base_out = base_in;               // logical base (gate records), output base
        if (P.chained) { base = fuse_deposit(t, P.seg_lg, P.nseg_lg); base_out = fuse_deposit(t, P.seg_out, P.nseg_out); }
        const amp_t *g = amp + (base_in | off_t);
        amp_t *go = amp_out + (base_out | st_t);
        if constexpr (GEN) gen_tile<BLOCK, 8>(GF, tile, gen_phot, gen_res, base, packT, packK);
        else if (!(P.dbg & 4u)) {
#pragma unroll
            for (unsigned k = 0; k < 8; k++)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + off_k[k]),
                                                 (__attribute__((address_space(3))) void *)(tile + k * BLOCK + wbase), 16, 0, 2);
        }
        if (!staged) {          // round 5: a workgroup usually takes ONE tile -- the table staging used to sit in front of its fill, a
            staged = true;      // memory latency per tile with nothing else in flight (the tables are read after the barrier below)
            for (unsigned b = threadIdx.x; b < P.dg_cnt * 48u; b += BLOCK) dg[P.dg_cnt + b] = dg_area[3u * P.dg_cnt + b];
        }
        if (!EXACT && threadIdx.x < P.dg_cnt) {           // E_out of this tile for every diagonal of the pass, while the fill is in flight
            const DiagInfo *info = reinterpret_cast<const DiagInfo *>(dg_area) + threadIdx.x;
            const uint32_t present = info->present;
            amp_t E; E.x = info->kc; E.y = info->ks;
#pragma unroll
            for (unsigned f = 0; f < 5; f++)
                if ((present >> f) & 1u) cmul_tol(E, dg_area[info->field_off[f] + (unsigned)((base >> (8u * f)) & 255u)]);
            dg[threadIdx.x] = E;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (!(P.dbg & 1u)) {
            for (unsigned i = 0; i < P.nops; i += 2) {
                const uint32_t a = ops[i].a;
                const unsigned rb[3] = {a & 0xffu, (a >> 8) & 0xffu, (a >> 16) & 0xffu};
                const unsigned nsteps = (a >> 24) & 3u;
                const uint32_t sA = ops[i + 1].type, sB = ops[i + 1].a, sC = (uint32_t)ops[i + 1].mask;
                const unsigned p = (unsigned)insert_zero(insert_zero(insert_zero(threadIdx.x, rb[0]), rb[1]), rb[2]);
                // (which register bit each step works on is a compile-time fact of the variant: see qround_run)
                const unsigned perm = (sA & 3u) | ((sB & 3u) << 2) | ((sC & 3u) << 4);
                switch (perm) {
                case 0x06: q3_run<2, 1, 0, EXACT>(tile, p, rb, nsteps, sA, sB, sC, dg, gtab); break;     // sA=2, sB=1, sC=0: descending (Q:682-689)
                case 0x12: q3_run<2, 0, 1, EXACT>(tile, p, rb, nsteps, sA, sB, sC, dg, gtab); break;
                case 0x09: q3_run<1, 2, 0, EXACT>(tile, p, rb, nsteps, sA, sB, sC, dg, gtab); break;
                case 0x21: q3_run<1, 0, 2, EXACT>(tile, p, rb, nsteps, sA, sB, sC, dg, gtab); break;
                case 0x18: q3_run<0, 2, 1, EXACT>(tile, p, rb, nsteps, sA, sB, sC, dg, gtab); break;
                default:   q3_run<0, 1, 2, EXACT>(tile, p, rb, nsteps, sA, sB, sC, dg, gtab); break;     // 0x24: ascending
                }
                __syncthreads();
            }
        }
        amp_t v[8];
        const double sc = (P.dbg & 1u) ? 1.0 : P.tol_scale;
#pragma unroll
        for (unsigned k = 0; k < 8; k++) {
            v[k] = tile[ld_k[k] | ld_t];                                    // (store order: ascending OUTPUT positions)
            if constexpr (EXACT) { v[k].x += 0.0; v[k].y += 0.0; }          // the reference's canonical zeros, once per pass
            else { v[k].x *= sc; v[k].y *= sc; }
        }
        if (!(P.dbg & 2u)) {
#pragma unroll
            for (unsigned k = 0; k < 8; k++) __builtin_nontemporal_store(v[k], go + st_k[k]);
        }
        __syncthreads();
    }
}


// ---------------------------------------------------------------------------
// K6x  the EXACT walk on 8 amplitudes per thread (round 5; bit-exact).  Same records, same per-amplitude arithmetic in the same
// order as the radix-4 rounds of k_fused_rounds -- a phase is the four products and two sums of rotate_amp without FMA, an H the
// butterfly of h_butterfly, the canonical "+ 0.0" once per round / run -- but a round carries THREE register bits: a thread keeps
// the 8 amplitudes that differ in them, three Hadamards and their phase runs cost one LDS round trip and one barrier, and a tile
// of 2^12 amplitudes needs 512 threads instead of 1024 (8 hot bits per pass next to c = 4: the n = 28 inverse QFT in 3 passes
// instead of 4).  Round 3 tried this in C++ and lost to the compiler's register copies (21 ms against 12); here the WHOLE round
// -- the eight LDS reads, the item loop, every rotation, the LDS writes -- is ONE asm statement on FIXED registers:
//     v[32:63]   the 8 amplitudes: register r (bit j of r = the round's register bit j) is x = v[32+4r : 33+4r], y = v[34+4r : 35+4r]
//     v[24:31]   four temporaries; v[20:21] this lane's outside-tile mask of the current item (the next item's is fetched into it
//                as soon as the current one has been tested); v18, v19 scratch
//     s[72:79] / s[80:87]  the two record blocks (one s_load_dwordx8 per gate, the next gate's in flight); s[88:89] the item
//     pointer; s[90:91] live gates of the run; s[92:93] saved EXEC; s94 scratch; s95 / s96 header of this / the next item;
//     s97 records left in the round; s98 gates of the item
// all named on the clobber list (the kernel is built for 4 waves per SIMD -- what its LDS tile allows anyway -- so they lie
// inside the allocator's budget).  Records of a round:
//   FUSE_ROUND8  a = rb0 | rb1 << 8 | rb2 << 16 | (round contains an H) << 24 | (no barrier needed in front of it) << 25,  mask = records that follow,
//                c (as 64 bits) = the tile-local bit that thread bit i rides on, 4 bits each (the lane and wave numbers are laid
//                over the non-register bits in the order the host likes best)
//   item H       type = FUSE_H | (32 | j) << 8                        H on register bit j
//   item run     type = FUSE_PRUN | (pat | canon << 4) << 8 | gates << 16   1..63 gates that rotate the same registers:
//                pat 0 = all eight; 1 / 2 / 3 = those with register bit 0 / 1 / 2 set; 4 / 5 / 6 = with bits {0,1} / {0,2} / {1,2} set
//   gate of run  as in the radix-4 form: a = tile-local mask without the register bits, mask = outside-tile bits, c, s; conditions on
//                the tile bits the round's wave number rides on sit in mask bits 48 .. (bit 48 + k: thread bit 6 + k)
// ---------------------------------------------------------------------------
enum : uint32_t { FUSE_ROUND8 = 9 };

#define X8X0 "v[32:33]"
#define X8Y0 "v[34:35]"
#define X8X1 "v[36:37]"
#define X8Y1 "v[38:39]"
#define X8X2 "v[40:41]"
#define X8Y2 "v[42:43]"
#define X8X3 "v[44:45]"
#define X8Y3 "v[46:47]"
#define X8X4 "v[48:49]"
#define X8Y4 "v[50:51]"
#define X8X5 "v[52:53]"
#define X8Y5 "v[54:55]"
#define X8X6 "v[56:57]"
#define X8Y6 "v[58:59]"
#define X8X7 "v[60:61]"
#define X8Y7 "v[62:63]"
#define X8T0 "v[24:25]"
#define X8T1 "v[26:27]"
#define X8T2 "v[28:29]"
#define X8T3 "v[30:31]"
// two rotations interleaved on the four temporaries (the same sequence as QCX_ROT2)
#define X8_ROT2(C, S, XA, YA, XB, YB)                                \
    "v_mul_f64 " X8T0 ", " C ", " XA "\n\t"                          \
    "v_mul_f64 " X8T1 ", " S ", " YA "\n\t"                          \
    "v_mul_f64 " X8T2 ", " C ", " YA "\n\t"                          \
    "v_mul_f64 " X8T3 ", " S ", " XA "\n\t"                          \
    "v_add_f64 " XA ", " X8T0 ", -" X8T1 "\n\t"                      \
    "v_mul_f64 " X8T0 ", " C ", " XB "\n\t"                          \
    "v_mul_f64 " X8T1 ", " S ", " YB "\n\t"                          \
    "v_add_f64 " YA ", " X8T2 ", " X8T3 "\n\t"                       \
    "v_mul_f64 " X8T2 ", " C ", " YB "\n\t"                          \
    "v_mul_f64 " X8T3 ", " S ", " XB "\n\t"                          \
    "v_add_f64 " XB ", " X8T0 ", -" X8T1 "\n\t"                      \
    "v_add_f64 " YB ", " X8T2 ", " X8T3 "\n\t"
#define X8_R2(C, S, i, j) X8_ROT2(C, S, X8X##i, X8Y##i, X8X##j, X8Y##j)
#define X8_ROTS_0(C, S) X8_R2(C, S, 0, 1) X8_R2(C, S, 2, 3) X8_R2(C, S, 4, 5) X8_R2(C, S, 6, 7)
#define X8_ROTS_1(C, S) X8_R2(C, S, 1, 3) X8_R2(C, S, 5, 7)
#define X8_ROTS_2(C, S) X8_R2(C, S, 2, 3) X8_R2(C, S, 6, 7)
#define X8_ROTS_3(C, S) X8_R2(C, S, 4, 5) X8_R2(C, S, 6, 7)
#define X8_ROTS_4(C, S) X8_R2(C, S, 3, 7)
#define X8_ROTS_5(C, S) X8_R2(C, S, 5, 7)
#define X8_ROTS_6(C, S) X8_R2(C, S, 6, 7)
#define X8_Z1(i) "v_add_f64 " X8X##i ", " X8X##i ", 0\n\t" "v_add_f64 " X8Y##i ", " X8Y##i ", 0\n\t"
#define X8_ZERO_0 X8_Z1(0) X8_Z1(1) X8_Z1(2) X8_Z1(3) X8_Z1(4) X8_Z1(5) X8_Z1(6) X8_Z1(7)
#define X8_ZERO_1 X8_Z1(1) X8_Z1(3) X8_Z1(5) X8_Z1(7)
#define X8_ZERO_2 X8_Z1(2) X8_Z1(3) X8_Z1(6) X8_Z1(7)
#define X8_ZERO_3 X8_Z1(4) X8_Z1(5) X8_Z1(6) X8_Z1(7)
#define X8_ZERO_4 X8_Z1(3) X8_Z1(7)
#define X8_ZERO_5 X8_Z1(5) X8_Z1(7)
#define X8_ZERO_6 X8_Z1(6) X8_Z1(7)
// H between registers A and B (A: the bit clear), without the final "+ 0.0" (the round canonicalises once at its end)
#define X8_HBF(A, B)                                                 \
    "v_mul_f64 " X8T0 ", %[hs], " X8X##A "\n\t"                      \
    "v_mul_f64 " X8T1 ", %[hs], " X8Y##A "\n\t"                      \
    "v_mul_f64 " X8T2 ", %[hs], " X8X##B "\n\t"                      \
    "v_mul_f64 " X8T3 ", %[hs], " X8Y##B "\n\t"                      \
    "v_add_f64 " X8X##A ", " X8T0 ", " X8T2 "\n\t"                   \
    "v_add_f64 " X8Y##A ", " X8T1 ", " X8T3 "\n\t"                   \
    "v_add_f64 " X8X##B ", " X8T0 ", -" X8T2 "\n\t"                  \
    "v_add_f64 " X8Y##B ", " X8T1 ", -" X8T3 "\n\t"
#define X8_LOADREC(BLK)                                              \
    "s_ff1_i32_b64 s94, s[90:91]\n\t"                                \
    "s_bitset0_b64 s[90:91], s94\n\t"                                \
    "s_lshl_b32 s94, s94, 5\n\t"                                     \
    "s_load_dwordx8 " BLK ", s[88:89], s94 offset:0x20\n\t"
// one gate: a tile-local mask word of 0 (the usual case: the target lies outside the tile or on a register bit) skips the lane
// mask and the EXEC round trip
#define X8_GATE(M, ROTS)                                             \
    "s_cmp_eq_u32 " M ", 0\n\t"                                      \
    "s_cbranch_scc1 6f\n\t"                                          \
    "v_and_b32 v18, " M ", %[p]\n\t"                                 \
    "v_cmpx_eq_u32_e32 vcc, " M ", v18\n\t"                          \
    "s_cbranch_execz 1f\n\t"                                         \
    ROTS                                                             \
    "1:\n\t"                                                         \
    "s_mov_b64 exec, s[92:93]\n\t"                                   \
    "s_branch 7f\n\t"                                                \
    "6:\n\t"                                                         \
    ROTS                                                             \
    "7:\n\t"
#define X8_RUN_BODY(R)                                               \
    X8_LOADREC("s[72:79]")                                           \
    "2:\n\t"                                                         \
    "s_waitcnt lgkmcnt(0)\n\t"                                       \
    "s_cmp_eq_u64 s[90:91], 0\n\t"                                   \
    "s_cbranch_scc1 3f\n\t"                                          \
    X8_LOADREC("s[80:87]")                                           \
    X8_GATE("s73", X8_ROTS_##R("s[76:77]", "s[78:79]"))              \
    "s_waitcnt lgkmcnt(0)\n\t"                                       \
    "s_cmp_eq_u64 s[90:91], 0\n\t"                                   \
    "s_cbranch_scc1 4f\n\t"                                          \
    X8_LOADREC("s[72:79]")                                           \
    X8_GATE("s81", X8_ROTS_##R("s[84:85]", "s[86:87]"))              \
    "s_branch 2b\n\t"                                                \
    "3:\n\t"                                                         \
    X8_GATE("s73", X8_ROTS_##R("s[76:77]", "s[78:79]"))              \
    "s_branch 5f\n\t"                                                \
    "4:\n\t"                                                         \
    X8_GATE("s81", X8_ROTS_##R("s[84:85]", "s[86:87]"))              \
    "5:\n\t"                                                         \
    "s_bitcmp1_b32 s95, 12\n\t"                                      \
    "s_cbranch_scc0 99f\n\t"                                         \
    X8_ZERO_##R                                                      \
    "s_branch 99f\n\t"
// address of register r's amplitude: a0 XOR the deltas of its set register bits (v19) -- XOR, not +: the tile sits in LDS under the
// swizzle x8_swz, which is linear over XOR
#define X8_ADDR1(D)        "v_xor_b32 v19, " D ", %[a0]\n\t"
#define X8_ADDR2(D, E)     "v_xor_b32 v19, " D ", %[a0]\n\t" "v_xor_b32 v19, " E ", v19\n\t"
#define X8_ADDR3(D, E, F)  "v_xor_b32 v19, " D ", %[a0]\n\t" "v_xor_b32 v19, " E ", v19\n\t" "v_xor_b32 v19, " F ", v19\n\t"
#define X8_ROUND_ALL                                                 \
    "s_mov_b64 s[88:89], %[item]\n\t"                                \
    "s_mov_b32 s97, %[cnt]\n\t"                                      \
    "s_load_dword s95, s[88:89], 0x0\n\t"                            \
    "ds_read_b64 v[20:21], %[xa]\n\t"                                \
    "ds_read_b128 v[32:35], %[a0]\n\t"                               \
    X8_ADDR1("%[d0]") "ds_read_b128 v[36:39], v19\n\t"               \
    X8_ADDR1("%[d1]") "ds_read_b128 v[40:43], v19\n\t"               \
    X8_ADDR2("%[d0]", "%[d1]") "ds_read_b128 v[44:47], v19\n\t"      \
    X8_ADDR1("%[d2]") "ds_read_b128 v[48:51], v19\n\t"               \
    X8_ADDR2("%[d0]", "%[d2]") "ds_read_b128 v[52:55], v19\n\t"      \
    X8_ADDR2("%[d1]", "%[d2]") "ds_read_b128 v[56:59], v19\n\t"      \
    X8_ADDR3("%[d0]", "%[d1]", "%[d2]") "ds_read_b128 v[60:63], v19\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t"                                       \
    /* ---- one item ---- */                                         \
    "90:\n\t"                                                        \
    "s_lshr_b32 s98, s95, 16\n\t"                                    \
    /* what the NEXT item needs first: its header dword and this lane's entry of its outside-tile masks */ \
    "s_add_u32 s94, s98, 1\n\t"                                      \
    "s_lshl_b32 s96, s94, 5\n\t"                                     \
    "s_load_dword s96, s[88:89], s96\n\t"                            \
    "v_lshl_add_u32 %[xa], s94, 3, %[xa]\n\t"                        \
    "s_bitcmp1_b32 s95, 13\n\t"                                      \
    "s_cbranch_scc1 50f\n\t"                                         \
    /* the run's live gates: lane l tests gate l's outside-tile controls against the tile's base */ \
    "v_and_b32 v18, %[blo], v20\n\t"                                 \
    "v_and_b32 v19, %[bhi], v21\n\t"                                 \
    "v_cmp_eq_u64_e64 s[90:91], v[18:19], v[20:21]\n\t"              \
    "ds_read_b64 v[20:21], %[xa]\n\t"                                \
    "s_bfm_b64 s[92:93], s98, 0\n\t"                                 \
    "s_and_b64 s[90:91], s[90:91], s[92:93]\n\t"                     \
    "s_mov_b64 s[92:93], exec\n\t"                                   \
    "s_cmp_eq_u64 s[90:91], 0\n\t"                                   \
    "s_cbranch_scc1 99f\n\t"                                         \
    "s_bfe_u32 s94, s95, 0x30008\n\t"                                \
    "s_cmp_lt_u32 s94, 4\n\t s_cbranch_scc1 40f\n\t"                 \
    "s_cmp_lt_u32 s94, 6\n\t s_cbranch_scc1 41f\n\t s_branch 26f\n\t" \
    "41:\n\t s_cmp_eq_u32 s94, 4\n\t s_cbranch_scc1 24f\n\t s_branch 25f\n\t" \
    "40:\n\t s_cmp_lt_u32 s94, 2\n\t s_cbranch_scc1 42f\n\t s_cmp_eq_u32 s94, 2\n\t s_cbranch_scc1 22f\n\t s_branch 23f\n\t" \
    "42:\n\t s_cmp_eq_u32 s94, 0\n\t s_cbranch_scc1 20f\n\t s_branch 21f\n\t" \
    "20:\n\t" X8_RUN_BODY(0) "21:\n\t" X8_RUN_BODY(1) "22:\n\t" X8_RUN_BODY(2) "23:\n\t" X8_RUN_BODY(3) \
    "24:\n\t" X8_RUN_BODY(4) "25:\n\t" X8_RUN_BODY(5) "26:\n\t" X8_RUN_BODY(6) \
    "50:\n\t"                                                        \
    "ds_read_b64 v[20:21], %[xa]\n\t"                                \
    "s_bfe_u32 s94, s95, 0x20008\n\t"                                \
    "s_cmp_eq_u32 s94, 0\n\t s_cbranch_scc1 51f\n\t"                 \
    "s_cmp_eq_u32 s94, 1\n\t s_cbranch_scc1 52f\n\t"                 \
    X8_HBF(0, 4) X8_HBF(1, 5) X8_HBF(2, 6) X8_HBF(3, 7)              \
    "s_branch 99f\n\t"                                               \
    "51:\n\t"                                                        \
    X8_HBF(0, 1) X8_HBF(2, 3) X8_HBF(4, 5) X8_HBF(6, 7)              \
    "s_branch 99f\n\t"                                               \
    "52:\n\t"                                                        \
    X8_HBF(0, 2) X8_HBF(1, 3) X8_HBF(4, 6) X8_HBF(5, 7)              \
    "99:\n\t"                                                        \
    "s_waitcnt lgkmcnt(0)\n\t"                                       \
    /* on to the next item */                                        \
    "s_add_u32 s94, s98, 1\n\t"                                      \
    "s_sub_u32 s97, s97, s94\n\t"                                    \
    "s_lshl_b32 s94, s94, 5\n\t"                                     \
    "s_add_u32 s88, s88, s94\n\t"                                    \
    "s_addc_u32 s89, s89, 0\n\t"                                     \
    "s_mov_b32 s95, s96\n\t"                                         \
    "s_cmp_lg_u32 s97, 0\n\t"                                        \
    "s_cbranch_scc1 90b\n\t"                                         \
    /* ---- end of the round: canonical zeros if it held an H, then the eight LDS writes ---- */ \
    "s_bitcmp1_b32 %[fl], 0\n\t"                                     \
    "s_cbranch_scc0 98f\n\t"                                         \
    X8_ZERO_0                                                        \
    "98:\n\t"                                                        \
    "ds_write_b128 %[a0], v[32:35]\n\t"                              \
    X8_ADDR1("%[d0]") "ds_write_b128 v19, v[36:39]\n\t"              \
    X8_ADDR1("%[d1]") "ds_write_b128 v19, v[40:43]\n\t"              \
    X8_ADDR2("%[d0]", "%[d1]") "ds_write_b128 v19, v[44:47]\n\t"     \
    X8_ADDR1("%[d2]") "ds_write_b128 v19, v[48:51]\n\t"              \
    X8_ADDR2("%[d0]", "%[d2]") "ds_write_b128 v19, v[52:55]\n\t"     \
    X8_ADDR2("%[d1]", "%[d2]") "ds_write_b128 v19, v[56:59]\n\t"     \
    X8_ADDR3("%[d0]", "%[d1]", "%[d2]") "ds_write_b128 v19, v[60:63]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t"

// The tile's LDS layout: element e lives in slot e ^ (bits 4-7 of e) ^ (bits 8-11 of e) -- the two upper nibbles folded onto the
// lowest.  A wave's 64 lanes ride on whatever six tile bits the host picked for the round (x8_assign_maps: bits that few gates of
// the round test), seldom the lowest six; unswizzled, lanes that differ only in high bits would share their 16-byte bank group
// (measured: 74 % of the LDS cycles of the first build were bank conflicts).  The map is an involution and linear over XOR, so
// the fill (LDS-DMA: slot s receives element x8_swz(s)), the rounds and the store all address through XOR of per-bit terms.
__device__ __forceinline__ uint32_t x8_swz(uint32_t e) { return e ^ ((e >> 4) & 15u) ^ ((e >> 8) & 15u); }

// one whole round of the exact walk on this thread's 8 amplitudes (see K6x above).  a0 = LDS byte address of the slot of element p;
// d0..d2 = what a set register bit XORs onto it; xaddr = LDS byte address of this lane's entry of the first item's outside-tile masks;
// item = the first item's record; cnt = records of the round; base = the tile's LOGICAL base index
__device__ __forceinline__ void fuse_round8(uint32_t a0, unsigned p, uint32_t xaddr, uint64_t base, const FuseOp *item, uint32_t cnt,
                                            uint32_t d0, uint32_t d1, uint32_t d2, uint32_t has_h)
{
    const double hs = QCX_SQRT1_2;
    const uint32_t blo = (uint32_t)base, bhi = (uint32_t)(base >> 32);
    asm volatile(X8_ROUND_ALL
        : [xa] "+v"(xaddr)
        : [a0] "v"(a0), [p] "v"(p), [blo] "s"(blo), [bhi] "s"(bhi), [item] "s"(item), [cnt] "s"(cnt),
          [d0] "s"(d0), [d1] "s"(d1), [d2] "s"(d2), [fl] "s"(has_h), [hs] "s"(hs)
        : "memory", "vcc", "scc",
          "v18", "v19", "v20", "v21", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31",
          "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47",
          "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63",
          "s72", "s73", "s74", "s75", "s76", "s77", "s78", "s79", "s80", "s81", "s82", "s83", "s84", "s85", "s86", "s87",
          "s88", "s89", "s90", "s91", "s92", "s93", "s94", "s95", "s96", "s97", "s98");
}


// ---------------------------------------------------------------------------
// K6x-t  TOLERANCE MODE on the same shell (round 5; opt-in, NOT bit-exact -- the arithmetic of K6t-8 / k_fused_q3, whose records it
// reads: FUSE_QROUND3 rounds of up to three steps H(x) [D(x)]).  k_fused_q3 is C++ and the compiler's version of a round copies the
// eight amplitudes between register sets (44 % of its vector instructions were moves: the pass was bound by them, 4.3 ms of
// arithmetic next to 4.6 ms of memory for the n = 28 inverse QFT).  Here a round is one asm statement on fixed registers:
//     v[32:63]   the 8 amplitudes; the unscaled butterfly of a pair works in place as a' = a + b, b' = a' - 2 b (an add and an FMA)
//     v[64:67]   F = E_out(tile) x the G-table entries of this thread's tile bits;  v[68:79] the entries, then F w1, F w2, F w1 w2
//     v[24:31]   w1, w2: the factors of the step's other two register bits ((1, 0) where the diagonal does not target them)
//     v[20:23]   temporaries, v19 an address
// The header of a round carries what FUSE_ROUND8 carries: the thread map in c (x8_assign_maps) and -- bit 28 of a -- "no barrier
// needed in front of this round".
// ---------------------------------------------------------------------------
// (generated by a small script: the butterflies of a step per register bit -- in place: a' = a + b, b' = a' - 2 b, one rounding
//  each, no second register set --, the diagonal of a step per register bit, F times a table entry)
#define X8T_H_0 \
    "v_add_f64 v[32:33], v[32:33], v[36:37]\n\t" \
    "v_fma_f64 v[36:37], -2.0, v[36:37], v[32:33]\n\t" \
    "v_add_f64 v[34:35], v[34:35], v[38:39]\n\t" \
    "v_fma_f64 v[38:39], -2.0, v[38:39], v[34:35]\n\t" \
    "v_add_f64 v[40:41], v[40:41], v[44:45]\n\t" \
    "v_fma_f64 v[44:45], -2.0, v[44:45], v[40:41]\n\t" \
    "v_add_f64 v[42:43], v[42:43], v[46:47]\n\t" \
    "v_fma_f64 v[46:47], -2.0, v[46:47], v[42:43]\n\t" \
    "v_add_f64 v[48:49], v[48:49], v[52:53]\n\t" \
    "v_fma_f64 v[52:53], -2.0, v[52:53], v[48:49]\n\t" \
    "v_add_f64 v[50:51], v[50:51], v[54:55]\n\t" \
    "v_fma_f64 v[54:55], -2.0, v[54:55], v[50:51]\n\t" \
    "v_add_f64 v[56:57], v[56:57], v[60:61]\n\t" \
    "v_fma_f64 v[60:61], -2.0, v[60:61], v[56:57]\n\t" \
    "v_add_f64 v[58:59], v[58:59], v[62:63]\n\t" \
    "v_fma_f64 v[62:63], -2.0, v[62:63], v[58:59]\n\t"
#define X8T_H_1 \
    "v_add_f64 v[32:33], v[32:33], v[40:41]\n\t" \
    "v_fma_f64 v[40:41], -2.0, v[40:41], v[32:33]\n\t" \
    "v_add_f64 v[34:35], v[34:35], v[42:43]\n\t" \
    "v_fma_f64 v[42:43], -2.0, v[42:43], v[34:35]\n\t" \
    "v_add_f64 v[36:37], v[36:37], v[44:45]\n\t" \
    "v_fma_f64 v[44:45], -2.0, v[44:45], v[36:37]\n\t" \
    "v_add_f64 v[38:39], v[38:39], v[46:47]\n\t" \
    "v_fma_f64 v[46:47], -2.0, v[46:47], v[38:39]\n\t" \
    "v_add_f64 v[48:49], v[48:49], v[56:57]\n\t" \
    "v_fma_f64 v[56:57], -2.0, v[56:57], v[48:49]\n\t" \
    "v_add_f64 v[50:51], v[50:51], v[58:59]\n\t" \
    "v_fma_f64 v[58:59], -2.0, v[58:59], v[50:51]\n\t" \
    "v_add_f64 v[52:53], v[52:53], v[60:61]\n\t" \
    "v_fma_f64 v[60:61], -2.0, v[60:61], v[52:53]\n\t" \
    "v_add_f64 v[54:55], v[54:55], v[62:63]\n\t" \
    "v_fma_f64 v[62:63], -2.0, v[62:63], v[54:55]\n\t"
#define X8T_H_2 \
    "v_add_f64 v[32:33], v[32:33], v[48:49]\n\t" \
    "v_fma_f64 v[48:49], -2.0, v[48:49], v[32:33]\n\t" \
    "v_add_f64 v[34:35], v[34:35], v[50:51]\n\t" \
    "v_fma_f64 v[50:51], -2.0, v[50:51], v[34:35]\n\t" \
    "v_add_f64 v[36:37], v[36:37], v[52:53]\n\t" \
    "v_fma_f64 v[52:53], -2.0, v[52:53], v[36:37]\n\t" \
    "v_add_f64 v[38:39], v[38:39], v[54:55]\n\t" \
    "v_fma_f64 v[54:55], -2.0, v[54:55], v[38:39]\n\t" \
    "v_add_f64 v[40:41], v[40:41], v[56:57]\n\t" \
    "v_fma_f64 v[56:57], -2.0, v[56:57], v[40:41]\n\t" \
    "v_add_f64 v[42:43], v[42:43], v[58:59]\n\t" \
    "v_fma_f64 v[58:59], -2.0, v[58:59], v[42:43]\n\t" \
    "v_add_f64 v[44:45], v[44:45], v[60:61]\n\t" \
    "v_fma_f64 v[60:61], -2.0, v[60:61], v[44:45]\n\t" \
    "v_add_f64 v[46:47], v[46:47], v[62:63]\n\t" \
    "v_fma_f64 v[62:63], -2.0, v[62:63], v[46:47]\n\t"
#define X8T_D_0 \
    "v_mul_f64 v[20:21], v[26:27], v[66:67]\n\t" \
    "v_mul_f64 v[70:71], v[26:27], v[64:65]\n\t" \
    "v_fma_f64 v[68:69], v[24:25], v[64:65], -v[20:21]\n\t" \
    "v_fma_f64 v[70:71], v[24:25], v[66:67], v[70:71]\n\t" \
    "v_mul_f64 v[20:21], v[30:31], v[66:67]\n\t" \
    "v_mul_f64 v[74:75], v[30:31], v[64:65]\n\t" \
    "v_fma_f64 v[72:73], v[28:29], v[64:65], -v[20:21]\n\t" \
    "v_fma_f64 v[74:75], v[28:29], v[66:67], v[74:75]\n\t" \
    "v_mul_f64 v[20:21], v[30:31], v[70:71]\n\t" \
    "v_mul_f64 v[78:79], v[30:31], v[68:69]\n\t" \
    "v_fma_f64 v[76:77], v[28:29], v[68:69], -v[20:21]\n\t" \
    "v_fma_f64 v[78:79], v[28:29], v[70:71], v[78:79]\n\t" \
    "v_mul_f64 v[20:21], v[66:67], v[38:39]\n\t" \
    "v_mul_f64 v[22:23], v[66:67], v[36:37]\n\t" \
    "v_fma_f64 v[36:37], v[64:65], v[36:37], -v[20:21]\n\t" \
    "v_fma_f64 v[38:39], v[64:65], v[38:39], v[22:23]\n\t" \
    "v_mul_f64 v[20:21], v[70:71], v[46:47]\n\t" \
    "v_mul_f64 v[22:23], v[70:71], v[44:45]\n\t" \
    "v_fma_f64 v[44:45], v[68:69], v[44:45], -v[20:21]\n\t" \
    "v_fma_f64 v[46:47], v[68:69], v[46:47], v[22:23]\n\t" \
    "v_mul_f64 v[20:21], v[74:75], v[54:55]\n\t" \
    "v_mul_f64 v[22:23], v[74:75], v[52:53]\n\t" \
    "v_fma_f64 v[52:53], v[72:73], v[52:53], -v[20:21]\n\t" \
    "v_fma_f64 v[54:55], v[72:73], v[54:55], v[22:23]\n\t" \
    "v_mul_f64 v[20:21], v[78:79], v[62:63]\n\t" \
    "v_mul_f64 v[22:23], v[78:79], v[60:61]\n\t" \
    "v_fma_f64 v[60:61], v[76:77], v[60:61], -v[20:21]\n\t" \
    "v_fma_f64 v[62:63], v[76:77], v[62:63], v[22:23]\n\t"
#define X8T_D_1 \
    "v_mul_f64 v[20:21], v[26:27], v[66:67]\n\t" \
    "v_mul_f64 v[70:71], v[26:27], v[64:65]\n\t" \
    "v_fma_f64 v[68:69], v[24:25], v[64:65], -v[20:21]\n\t" \
    "v_fma_f64 v[70:71], v[24:25], v[66:67], v[70:71]\n\t" \
    "v_mul_f64 v[20:21], v[30:31], v[66:67]\n\t" \
    "v_mul_f64 v[74:75], v[30:31], v[64:65]\n\t" \
    "v_fma_f64 v[72:73], v[28:29], v[64:65], -v[20:21]\n\t" \
    "v_fma_f64 v[74:75], v[28:29], v[66:67], v[74:75]\n\t" \
    "v_mul_f64 v[20:21], v[30:31], v[70:71]\n\t" \
    "v_mul_f64 v[78:79], v[30:31], v[68:69]\n\t" \
    "v_fma_f64 v[76:77], v[28:29], v[68:69], -v[20:21]\n\t" \
    "v_fma_f64 v[78:79], v[28:29], v[70:71], v[78:79]\n\t" \
    "v_mul_f64 v[20:21], v[66:67], v[42:43]\n\t" \
    "v_mul_f64 v[22:23], v[66:67], v[40:41]\n\t" \
    "v_fma_f64 v[40:41], v[64:65], v[40:41], -v[20:21]\n\t" \
    "v_fma_f64 v[42:43], v[64:65], v[42:43], v[22:23]\n\t" \
    "v_mul_f64 v[20:21], v[70:71], v[46:47]\n\t" \
    "v_mul_f64 v[22:23], v[70:71], v[44:45]\n\t" \
    "v_fma_f64 v[44:45], v[68:69], v[44:45], -v[20:21]\n\t" \
    "v_fma_f64 v[46:47], v[68:69], v[46:47], v[22:23]\n\t" \
    "v_mul_f64 v[20:21], v[74:75], v[58:59]\n\t" \
    "v_mul_f64 v[22:23], v[74:75], v[56:57]\n\t" \
    "v_fma_f64 v[56:57], v[72:73], v[56:57], -v[20:21]\n\t" \
    "v_fma_f64 v[58:59], v[72:73], v[58:59], v[22:23]\n\t" \
    "v_mul_f64 v[20:21], v[78:79], v[62:63]\n\t" \
    "v_mul_f64 v[22:23], v[78:79], v[60:61]\n\t" \
    "v_fma_f64 v[60:61], v[76:77], v[60:61], -v[20:21]\n\t" \
    "v_fma_f64 v[62:63], v[76:77], v[62:63], v[22:23]\n\t"
#define X8T_D_2 \
    "v_mul_f64 v[20:21], v[26:27], v[66:67]\n\t" \
    "v_mul_f64 v[70:71], v[26:27], v[64:65]\n\t" \
    "v_fma_f64 v[68:69], v[24:25], v[64:65], -v[20:21]\n\t" \
    "v_fma_f64 v[70:71], v[24:25], v[66:67], v[70:71]\n\t" \
    "v_mul_f64 v[20:21], v[30:31], v[66:67]\n\t" \
    "v_mul_f64 v[74:75], v[30:31], v[64:65]\n\t" \
    "v_fma_f64 v[72:73], v[28:29], v[64:65], -v[20:21]\n\t" \
    "v_fma_f64 v[74:75], v[28:29], v[66:67], v[74:75]\n\t" \
    "v_mul_f64 v[20:21], v[30:31], v[70:71]\n\t" \
    "v_mul_f64 v[78:79], v[30:31], v[68:69]\n\t" \
    "v_fma_f64 v[76:77], v[28:29], v[68:69], -v[20:21]\n\t" \
    "v_fma_f64 v[78:79], v[28:29], v[70:71], v[78:79]\n\t" \
    "v_mul_f64 v[20:21], v[66:67], v[50:51]\n\t" \
    "v_mul_f64 v[22:23], v[66:67], v[48:49]\n\t" \
    "v_fma_f64 v[48:49], v[64:65], v[48:49], -v[20:21]\n\t" \
    "v_fma_f64 v[50:51], v[64:65], v[50:51], v[22:23]\n\t" \
    "v_mul_f64 v[20:21], v[70:71], v[54:55]\n\t" \
    "v_mul_f64 v[22:23], v[70:71], v[52:53]\n\t" \
    "v_fma_f64 v[52:53], v[68:69], v[52:53], -v[20:21]\n\t" \
    "v_fma_f64 v[54:55], v[68:69], v[54:55], v[22:23]\n\t" \
    "v_mul_f64 v[20:21], v[74:75], v[58:59]\n\t" \
    "v_mul_f64 v[22:23], v[74:75], v[56:57]\n\t" \
    "v_fma_f64 v[56:57], v[72:73], v[56:57], -v[20:21]\n\t" \
    "v_fma_f64 v[58:59], v[72:73], v[58:59], v[22:23]\n\t" \
    "v_mul_f64 v[20:21], v[78:79], v[62:63]\n\t" \
    "v_mul_f64 v[22:23], v[78:79], v[60:61]\n\t" \
    "v_fma_f64 v[60:61], v[76:77], v[60:61], -v[20:21]\n\t" \
    "v_fma_f64 v[62:63], v[76:77], v[62:63], v[22:23]\n\t"
#define X8T_FMUL_0 \
    "v_mul_f64 v[20:21], v[70:71], v[66:67]\n\t" \
    "v_mul_f64 v[22:23], v[70:71], v[64:65]\n\t" \
    "v_fma_f64 v[64:65], v[68:69], v[64:65], -v[20:21]\n\t" \
    "v_fma_f64 v[66:67], v[68:69], v[66:67], v[22:23]\n\t"
#define X8T_FMUL_1 \
    "v_mul_f64 v[20:21], v[74:75], v[66:67]\n\t" \
    "v_mul_f64 v[22:23], v[74:75], v[64:65]\n\t" \
    "v_fma_f64 v[64:65], v[72:73], v[64:65], -v[20:21]\n\t" \
    "v_fma_f64 v[66:67], v[72:73], v[66:67], v[22:23]\n\t"
#define X8T_FMUL_2 \
    "v_mul_f64 v[20:21], v[78:79], v[66:67]\n\t" \
    "v_mul_f64 v[22:23], v[78:79], v[64:65]\n\t" \
    "v_fma_f64 v[64:65], v[76:77], v[64:65], -v[20:21]\n\t" \
    "v_fma_f64 v[66:67], v[76:77], v[66:67], v[22:23]\n\t"
#define X8T_STEP(K1, SW, NEXT)                                  \
    "s_cmp_lt_u32 %[ns], " #K1 "\n\t"                               \
    "s_cbranch_scc1 " NEXT "\n\t"                                    \
    "s_and_b32 s94, " SW ", 3\n\t"                                   \
    "s_bitcmp1_b32 " SW ", 2\n\t"                                    \
    "s_cbranch_scc0 60f\n\t"                                         \
    /* the diagonal's table reads, issued in front of the butterflies */ \
    "s_bfe_u32 s95, " SW ", 0x80008\n\t"                             \
    "s_lshl_b32 s96, s95, 4\n\t"                                     \
    "s_add_u32 s96, s96, %[dg]\n\t"                                  \
    "v_mov_b32 v19, s96\n\t"                                         \
    "ds_read_b128 v[64:67], v19\n\t"                                 \
    "s_mulk_i32 s95, 0x300\n\t"                                      \
    "s_add_u32 s95, s95, %[gt]\n\t"                                  \
    "s_bitcmp1_b32 " SW ", 16\n\t"                                   \
    "s_cbranch_scc0 61f\n\t"                                         \
    "v_add_u32 v19, s95, %[n0]\n\t"                                  \
    "ds_read_b128 v[68:71], v19\n\t"                               \
    "61:\n\t"                                                        \
    "s_bitcmp1_b32 " SW ", 17\n\t"                                   \
    "s_cbranch_scc0 62f\n\t"                                         \
    "v_add_u32 v19, s95, %[n1]\n\t"                                  \
    "ds_read_b128 v[72:75], v19\n\t"                               \
    "62:\n\t"                                                        \
    "s_bitcmp1_b32 " SW ", 18\n\t"                                   \
    "s_cbranch_scc0 63f\n\t"                                         \
    "v_add_u32 v19, s95, %[n2]\n\t"                                  \
    "ds_read_b128 v[76:79], v19\n\t"                               \
    "63:\n\t"                                                        \
    /* the other two register bits of the step: O1 = (R == 0 ? bit 1 : bit 0), O2 = (R == 2 ? bit 1 : bit 2) */ \
    "s_cmp_eq_u32 s94, 0\n\t"                                        \
    "s_cselect_b32 s97, %[o1], %[o0]\n\t"                            \
    "s_cmp_eq_u32 s94, 2\n\t"                                        \
    "s_cselect_b32 s98, %[o1], %[o2]\n\t"                            \
    "v_mov_b64 v[24:25], 1.0\n\t"                                    \
    "v_mov_b64 v[26:27], 0\n\t"                                      \
    "s_bitcmp1_b32 " SW ", 19\n\t"                                   \
    "s_cbranch_scc0 64f\n\t"                                         \
    "s_add_u32 s97, s97, s95\n\t"                                    \
    "v_mov_b32 v19, s97\n\t"                                         \
    "ds_read_b128 v[24:27], v19\n\t"                                 \
    "64:\n\t"                                                        \
    "v_mov_b64 v[28:29], 1.0\n\t"                                    \
    "v_mov_b64 v[30:31], 0\n\t"                                      \
    "s_bitcmp1_b32 " SW ", 20\n\t"                                   \
    "s_cbranch_scc0 60f\n\t"                                         \
    "s_add_u32 s98, s98, s95\n\t"                                    \
    "v_mov_b32 v19, s98\n\t"                                         \
    "ds_read_b128 v[28:31], v19\n\t"                                 \
    "60:\n\t"                                                        \
    /* the butterflies (unscaled: the pass multiplies by 1/sqrt 2 ^ Hadamards once, at the store) */ \
    "s_cmp_eq_u32 s94, 0\n\t s_cbranch_scc1 70f\n\t"                 \
    "s_cmp_eq_u32 s94, 1\n\t s_cbranch_scc1 71f\n\t"                 \
    X8T_H_2 "s_branch 72f\n\t"                                       \
    "70:\n\t" X8T_H_0 "s_branch 72f\n\t"                             \
    "71:\n\t" X8T_H_1                                                \
    "72:\n\t"                                                        \
    "s_bitcmp1_b32 " SW ", 2\n\t"                                    \
    "s_cbranch_scc0 " NEXT "\n\t"                                    \
    "s_waitcnt lgkmcnt(0)\n\t"                                       \
    "s_bitcmp1_b32 " SW ", 16\n\t s_cbranch_scc0 65f\n\t" X8T_FMUL_0 "65:\n\t" \
    "s_bitcmp1_b32 " SW ", 17\n\t s_cbranch_scc0 66f\n\t" X8T_FMUL_1 "66:\n\t" \
    "s_bitcmp1_b32 " SW ", 18\n\t s_cbranch_scc0 67f\n\t" X8T_FMUL_2 "67:\n\t" \
    "s_cmp_eq_u32 s94, 0\n\t s_cbranch_scc1 73f\n\t"                 \
    "s_cmp_eq_u32 s94, 1\n\t s_cbranch_scc1 74f\n\t"                 \
    X8T_D_2 "s_branch " NEXT "\n\t"                                  \
    "73:\n\t" X8T_D_0 "s_branch " NEXT "\n\t"                        \
    "74:\n\t" X8T_D_1
#define X8T_ROUND_ALL                                                \
    "ds_read_b128 v[32:35], %[a0]\n\t"                               \
    X8_ADDR1("%[d0]") "ds_read_b128 v[36:39], v19\n\t"               \
    X8_ADDR1("%[d1]") "ds_read_b128 v[40:43], v19\n\t"               \
    X8_ADDR2("%[d0]", "%[d1]") "ds_read_b128 v[44:47], v19\n\t"      \
    X8_ADDR1("%[d2]") "ds_read_b128 v[48:51], v19\n\t"               \
    X8_ADDR2("%[d0]", "%[d2]") "ds_read_b128 v[52:55], v19\n\t"      \
    X8_ADDR2("%[d1]", "%[d2]") "ds_read_b128 v[56:59], v19\n\t"      \
    X8_ADDR3("%[d0]", "%[d1]", "%[d2]") "ds_read_b128 v[60:63], v19\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t"                                       \
    X8T_STEP(1, "%[sA]", "81f") "81:\n\t"                            \
    X8T_STEP(2, "%[sB]", "82f") "82:\n\t"                            \
    X8T_STEP(3, "%[sC]", "83f") "83:\n\t"                            \
    "ds_write_b128 %[a0], v[32:35]\n\t"                              \
    X8_ADDR1("%[d0]") "ds_write_b128 v19, v[36:39]\n\t"              \
    X8_ADDR1("%[d1]") "ds_write_b128 v19, v[40:43]\n\t"              \
    X8_ADDR2("%[d0]", "%[d1]") "ds_write_b128 v19, v[44:47]\n\t"     \
    X8_ADDR1("%[d2]") "ds_write_b128 v19, v[48:51]\n\t"              \
    X8_ADDR2("%[d0]", "%[d2]") "ds_write_b128 v19, v[52:55]\n\t"     \
    X8_ADDR2("%[d1]", "%[d2]") "ds_write_b128 v19, v[56:59]\n\t"     \
    X8_ADDR3("%[d0]", "%[d1]", "%[d2]") "ds_write_b128 v19, v[60:63]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t"

// one fast round of the tolerance mode on this thread's 8 amplitudes.  n0..n2: byte offsets of this thread's entries in the three
// 16-entry groups of a diagonal's G tables (from its tile-local index p); o0..o2: byte offsets of the single-bit entries of the
// round's three register bits; dg / gt: LDS byte addresses of the E_out slots / the G tables
__device__ __forceinline__ void fuse_round8t(uint32_t a0, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t n0, uint32_t n1, uint32_t n2,
                                             uint32_t o0, uint32_t o1, uint32_t o2, uint32_t sA, uint32_t sB, uint32_t sC, uint32_t ns,
                                             uint32_t dg, uint32_t gt)
{
    asm volatile(X8T_ROUND_ALL
        :
        : [a0] "v"(a0), [d0] "s"(d0), [d1] "s"(d1), [d2] "s"(d2), [n0] "v"(n0), [n1] "v"(n1), [n2] "v"(n2),
          [o0] "s"(o0), [o1] "s"(o1), [o2] "s"(o2), [sA] "s"(sA), [sB] "s"(sB), [sC] "s"(sC), [ns] "s"(ns), [dg] "s"(dg), [gt] "s"(gt)
        : "memory", "vcc", "scc", "v19", "v20", "v21", "v22", "v23",
          "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31",
          "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47",
          "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63",
          "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79",
          "s94", "s95", "s96", "s97", "s98");
}

template <int BLOCK, int TT, bool GEN = false, bool TOL = false>     // TOL: the pass holds FUSE_QROUND3 rounds (tolerance mode, K6x-t)
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(4))) void k_fused_x8(
    const amp_t *amp, amp_t *amp_out, unsigned n, FusePass P, const FuseOp *__restrict__ ops, uint64_t ntiles, const FuseOp *ops_asm)
{
    static_assert((1u << TT) == 8u * BLOCK, "the walk on 8 amplitudes per thread");
    extern __shared__ __attribute__((aligned(16))) unsigned char qcx_lds_raw[];
    amp_t *tile = reinterpret_cast<amp_t *>(qcx_lds_raw);
    constexpr unsigned tsize = 1u << TT;
    uint64_t *xm = reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(tile + tsize) + P.xm_off);
    // tolerance mode: [E_out slot per diagonal][G tables, 48 entries per diagonal] behind the tile
    amp_t *dg = reinterpret_cast<amp_t *>(reinterpret_cast<unsigned char *>(tile + tsize) + P.dg_lds_off);
    const amp_t *dg_area = reinterpret_cast<const amp_t *>(ops + P.dg_rec_off);             // global: DiagInfo[], G tables, field tables
    bool staged = false;
    // fill: slot s = k * BLOCK + thread (what the LDS-DMA writes linearly) receives element x8_swz(s); spread and swizzle are both
    // linear over XOR, so the thread part and the k part are computed once and combined with XOR
    const uint64_t off_t = fuse_spread(x8_swz(threadIdx.x), P.in_pos, TT);
    uint64_t off_k[8], st_k[8];
    unsigned ld_k[8];
#pragma unroll
    for (unsigned k = 0; k < 8; k++) {
        off_k[k] = fuse_spread(x8_swz(k * BLOCK), P.in_pos, TT);
        st_k[k] = fuse_spread(k * BLOCK, P.st_pos, TT);
        ld_k[k] = x8_swz((unsigned)fuse_spread(k * BLOCK, P.st_loc, TT));
    }
    const uint64_t st_t = fuse_spread(threadIdx.x, P.st_pos, TT);
    const unsigned ld_t = x8_swz((unsigned)fuse_spread(threadIdx.x, P.st_loc, TT));
    const unsigned wbase = (threadIdx.x >> 6) * 64, lane = threadIdx.x & 63u;
    const unsigned wave_id = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t tile_lds = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) amp_t *)tile;
    const uint32_t xm_lds = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint64_t *)xm;
    const uint32_t dg_lds = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) amp_t *)dg;
    // the expanding store of a compact chain's last pass (FusePass::xp_on): this thread's share of an expanded store index --
    // its M-register value f (BLOCK >= 2^M: the same in every store), hence its column, and the thread bits above f
    uint64_t xp_off_t = 0;
    unsigned xp_slot_t = 0;
    bool xp_live = false;
    if (!GEN && P.xp_on) {
        const unsigned M = P.xp_M, f = threadIdx.x & ((1u << M) - 1u);
        unsigned col = 0xffu;
        for (unsigned j = 0; j < P.xp_ncols; j++) if (P.xp_orbit[j] == f) col = j;
        xp_live = col != 0xffu;
        unsigned loc = 0;
        if (xp_live) for (unsigned b = 0; b < P.xp_cb; b++) loc |= ((col >> b) & 1u) << P.xp_colloc[b];
        xp_off_t = f;
        for (unsigned i = M; (1u << i) < (unsigned)BLOCK; i++)
            if ((threadIdx.x >> i) & 1u) { xp_off_t |= (uint64_t)1 << P.xp_pos[i]; loc |= 1u << P.xp_loc[i]; }
        xp_slot_t = x8_swz(loc);
    }
    // GEN: the tiles are generated (the circuit front on a basis state that was never written, GenFront), not read: slot s holds
    // element x8_swz(s), and the per-element words of the generated fill are linear over XOR like everything else here
    const GenFront *GF = reinterpret_cast<const GenFront *>(ops + P.gen_rec_off);
    unsigned short *gen_phot = reinterpret_cast<unsigned short *>(reinterpret_cast<unsigned char *>(tile + tsize) + P.gen_lds_off);
    unsigned short *gen_res = gen_phot + 1024;
    uint32_t packT = 0, packK[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (GEN) {
        gen_setup<BLOCK>(GF, gen_phot);
        packT = gen_pack(x8_swz(threadIdx.x), GF, TT);
#pragma unroll
        for (unsigned k = 0; k < 8; k++) packK[k] = gen_pack(x8_swz(k * BLOCK), GF, TT);
        __syncthreads();
    }
    const unsigned slog = (P.dbg >> 12) & 15u;
    for (uint64_t b0 = blockIdx.x; b0 < ntiles; b0 += gridDim.x) {
        const uint64_t t = fuse_stream_tile(b0, n - TT, slog, (P.dbg >> 16) & 31u);
        const uint64_t base_in = fuse_deposit(t, P.seg_in, P.nseg_in);
        uint64_t base = base_in, base_out = base_in;               // logical base (gate records), output base
        if (P.chained) { base = fuse_deposit(t, P.seg_lg, P.nseg_lg); base_out = fuse_deposit(t, P.seg_out, P.nseg_out); }
        const amp_t *g = amp + base_in;
        amp_t *go = amp_out + (base_out | st_t);
        if constexpr (GEN) gen_tile<BLOCK, 8>(GF, tile, gen_phot, gen_res, base, packT, packK);
        else if (!(P.dbg & 4u)) {
#pragma unroll
            for (unsigned k = 0; k < 8; k++)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + (off_t ^ off_k[k])),
                                                 (__attribute__((address_space(3))) void *)(tile + k * BLOCK + wbase), 16, 0, 2);
        }
        if (!staged) {          // once per workgroup -- behind the first tile's fill, not in front of it (a workgroup usually takes ONE
            staged = true;      // tile: this latency used to be paid per tile, with nothing in flight)
            if constexpr (TOL) {
                for (unsigned b = threadIdx.x; b < P.dg_cnt * 48u; b += BLOCK) dg[P.dg_cnt + b] = dg_area[3u * P.dg_cnt + b];
            } else {            // the records' outside-tile masks (+ padding: a lane looks up to 64 entries past a run)
                for (unsigned b = threadIdx.x; b < P.xm_cnt + 66u; b += BLOCK) xm[b] = b < P.xm_cnt ? ops[b].mask : 0;
            }
        }
        if constexpr (TOL) {
            if (threadIdx.x < P.dg_cnt) {           // E_out of this tile for every diagonal of the pass, while the fill is in flight
                const DiagInfo *info = reinterpret_cast<const DiagInfo *>(dg_area) + threadIdx.x;
                const uint32_t present = info->present;
                amp_t E; E.x = info->kc; E.y = info->ks;
#pragma unroll
                for (unsigned f = 0; f < 5; f++)
                    if ((present >> f) & 1u) cmul_tol(E, dg_area[info->field_off[f] + (unsigned)((base >> (8u * f)) & 255u)]);
                dg[threadIdx.x] = E;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // Which part of the tile a wave takes through the rounds rotates with the tile number: gates whose condition sits on a
        // wave bit are skipped by the waves whose bit is 0, so the parts differ in work (part 7 of a pass with three filler
        // targets under the wave number runs 24 more gates than part 0), a wave sits on one SIMD for good, and a workgroup
        // lasts as long as its slowest wave -- with a fixed assignment one SIMD of every CU would carry the heavy parts of
        // BOTH resident workgroups.  (Fill and store go by the real thread number.)
        const unsigned wave_eff = TOL ? wave_id : (wave_id ^ (unsigned)t ^ (unsigned)(t >> 3)) & ((BLOCK >> 6) - 1u);
        const unsigned tid_eff = lane | (wave_eff << 6);
        if (!(P.dbg & 1u)) {
            for (unsigned i = 0; i < P.nops;) {
                const uint32_t a = ops[i].a;
                const unsigned rb0 = a & 0xffu, rb1 = (a >> 8) & 0xffu, rb2 = (a >> 16) & 0xffu;
                const uint32_t cnt = (uint32_t)ops[i].mask;
                uint64_t map; memcpy(&map, &ops[i].c, sizeof map);
                unsigned p = 0;
#pragma unroll
                for (unsigned k = 0; k < (unsigned)TT - 3u; k++) p |= ((tid_eff >> k) & 1u) << ((unsigned)(map >> (4u * k)) & 15u);
                // "no barrier in front of this round" (bit 25 of an exact round's header, bit 28 of a tolerance round's): its waves sit
                // on the same tile bits as the previous round's -- every wave finds its own amplitudes where it left them (its LDS
                // accesses are served in order) and nobody else's
                if (i != 0 && !((a >> (TOL ? 28 : 25)) & 1u)) __syncthreads();
                if constexpr (TOL) {
                    const uint32_t sA = ops[i + 1].type, sB = ops[i + 1].a, sC = (uint32_t)ops[i + 1].mask;
                    auto single = [](unsigned rb) { return 16u * (16u * (rb >> 2) + (1u << (rb & 3u))); };     // G-table entry of one tile bit alone
                    fuse_round8t(tile_lds + 16u * x8_swz(p), 16u * x8_swz(1u << rb0), 16u * x8_swz(1u << rb1), 16u * x8_swz(1u << rb2),
                                 16u * (p & 15u), 16u * (16u + ((p >> 4) & 15u)), 16u * (32u + (p >> 8)), single(rb0), single(rb1), single(rb2),
                                 sA, sB, sC, (a >> 24) & 3u, dg_lds, dg_lds + 16u * P.dg_cnt);
                } else {
                    // the walk reads the records through ops_asm (see fuse_apply_rounds: `ops` itself must not be captured by an asm)
                    // (bits 48 .. of a gate's outside mask: conditions on the tile bits this round's WAVE number rides on -- the host moved
                    //  them there from the lane mask, x8_assign_maps -- so that the per-item ballot already drops the gates this wave skips)
                    fuse_round8(tile_lds + 16u * x8_swz(p), p, xm_lds + 8u * (i + 2u + lane), base | ((uint64_t)wave_eff << 48), ops_asm + i + 1, cnt,
                                16u * x8_swz(1u << rb0), 16u * x8_swz(1u << rb1), 16u * x8_swz(1u << rb2), (a >> 24) & 1u);
                }
                i += 1 + cnt;
            }
            __syncthreads();
        }
        amp_t v[8];
        const double sc = (TOL && !(P.dbg & 1u)) ? P.tol_scale : 1.0;        // tolerance mode: the Hadamards' 1/sqrt 2, once per pass
        if (!GEN && P.xp_on) {
            // the real register from the compact tile: 2^(T - cb + M) amplitudes, store index e = it * BLOCK + thread; consecutive
            // threads write consecutive amplitudes (whole 2^M-blocks, runs of 2^(M + c - cb) of them), the threads whose f is on
            // the orbit fetch theirs from the tile, all others write +0
            constexpr unsigned LB = TT - 3u;                                 // log2 BLOCK
            const unsigned ebits = (unsigned)TT - P.xp_cb + P.xp_M, nit = 1u << (ebits - LB);
            amp_t *gx = amp_out + (((base_out >> P.xp_cb) << P.xp_M) | xp_off_t);
            for (unsigned it0 = 0; it0 < nit; it0 += 8) {
                uint64_t oi[8];
#pragma unroll
                for (unsigned k = 0; k < 8; k++) {
                    const unsigned it = it0 + k;
                    uint64_t off = 0; unsigned loc = 0;
                    for (unsigned b = 0; b < ebits - LB; b++)
                        if ((it >> b) & 1u) { off |= (uint64_t)1 << P.xp_pos[LB + b]; loc |= 1u << P.xp_loc[LB + b]; }
                    oi[k] = off;
                    v[k].x = 0.0; v[k].y = 0.0;
                    if (xp_live) { v[k] = tile[xp_slot_t ^ x8_swz(loc)]; if constexpr (TOL) { v[k].x *= sc; v[k].y *= sc; } }
                }
                if (!(P.dbg & 2u)) {
#pragma unroll
                    for (unsigned k = 0; k < 8; k++) if (it0 + k < nit) __builtin_nontemporal_store(v[k], gx + oi[k]);
                }
            }
            __syncthreads();
            continue;
        }
#pragma unroll
        for (unsigned k = 0; k < 8; k++) {
            v[k] = tile[ld_k[k] ^ ld_t];          // (store order: ascending OUTPUT positions; slots under the swizzle)
            if constexpr (TOL) { v[k].x *= sc; v[k].y *= sc; }
        }
        if (!(P.dbg & 2u)) {
#pragma unroll
            for (unsigned k = 0; k < 8; k++) __builtin_nontemporal_store(v[k], go + st_k[k]);
        }
        __syncthreads();
    }
}

// (A persistent, double-buffered form of the pass -- the LDS-DMA fill of tile i+1 in flight while tile i is processed and
// stored, the wait before use a COUNTED s_waitcnt vmcnt(stores issued after the fill) -- existed in round 1 and is gone:
// measured slower than this kernel, and the counted wait is not safe on gfx950.  A wave's loads and stores do not
// complete in one common order, so "all but the N youngest" may leave some of the older LOADS outstanding while the
// younger stores have already been acknowledged; round 2 saw exactly that as wrong amplitudes at n = 28 in a
// register-prefetch variant of an all-Hadamard pass, and the compiler itself always waits vmcnt(0) when loads and
// stores of one wave are pending together.  A wave that has stores in flight can only wait for ALL of its
// vector-memory operations; DESIGN.md s4 has the numbers of that experiment.)

// ---------------------------------------------------------------------------
// K0b  the circuit front on a BASIS state, in one write pass.  After reset_register (Q:318-324) -- or a measurement's
// collapse (Q:302-303) -- the register holds one amplitude (1, 0) at index b.  A prefix of the queued gates of the shape
//     H on distinct qubits (the set Hm)  then  controlled modular multiplies          (Q:720-731 is exactly that)
// has a closed form with the reference's own roundings:
//   * each H multiplies the populated amplitudes by s = M_SQRT1_2 ONCE MORE (the pair partner is an exact zero, so the
//     reference's (s*a +/- s*0) + 0 is fl(s*a) with sign -1 on the "1" side when the basis bit was 1): after k of them
//     every populated amplitude is +/- v_k, v_k = fl(s * v_(k-1)), v_0 = 1, sign = parity of (i & b & Hm);
//   * a modular multiply moves the one populated residue f of every 2^M block to (A f) mod C when its control bit is 1
//     and f < C (all other sources of that destination are exact zeros: 0 + ... + v = v), so after the ladder block x
//     holds its amplitude at f(x), the chain over the gates in issue order.
// The kernel writes EVERY amplitude of the shard once (the zeros too: it replaces the 16 * 2^n-byte memset of the reset),
// 16 * 2^n bytes instead of one read + write per Hadamard pass.  A wave owns 64 blocks: lane l walks the chain of block l,
// then the wave writes the 64 * 2^M amplitudes with coalesced 1-KiB stores, fetching each store's residues by shuffle.
// ---------------------------------------------------------------------------
struct BasisFront {
    uint64_t first;                         // global index of the shard's amplitude 0 (0 for an unsharded register)
    uint64_t basis, hmask, fixed_mask;      // populated blocks: (i & fixed_mask) == (basis & fixed_mask)
    uint64_t sign_mask;                     // sign = parity of popcount(i & sign_mask)
    double   v;                             // magnitude after the Hadamards
    unsigned M, ncam;                       // M = 0 and ncam = 0: no block structure (every amplitude is its own block)
    uint32_t C[64], A[64];
    uint8_t  ctl[64];
};

// the same rule, one thread per amplitude, for registers too small for a wave tile (n < M + 6: the reference's own sizes,
// e.g. L = 3, M = 4): every thread walks the residue chain of its block itself -- a few thousand amplitudes at most
__global__ __launch_bounds__(256) void k_basis_front_small(amp_t *__restrict__ amp, unsigned n, BasisFront B)
{
    const unsigned M = B.M;
    const uint64_t lowmask = ((uint64_t)1 << M) - 1;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < ((uint64_t)1 << n); i += (uint64_t)gridDim.x * 256) {
        const uint64_t gi = B.first + i, bi = gi & ~lowmask;
        unsigned f = (unsigned)(B.basis & lowmask);
        for (unsigned g = 0; g < B.ncam; g++)
            if (((bi >> B.ctl[g]) & 1u) && f < B.C[g]) f = (B.A[g] * f) % B.C[g];
        const unsigned low = (unsigned)(gi & lowmask), free_low = (unsigned)(B.hmask & lowmask);
        amp_t v; v.x = 0.0; v.y = 0.0;
        if ((bi & B.fixed_mask) == (B.basis & B.fixed_mask) && ((low ^ f) & ~free_low) == 0)
            v.x = (__builtin_popcountll(gi & B.sign_mask) & 1) ? -B.v : B.v;
        amp[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_basis_front(amp_t *__restrict__ amp, unsigned n, BasisFront B)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned M = B.M;
    const uint64_t ntiles = ((uint64_t)1 << n) >> (6 + M);          // host guarantees n >= M + 6
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = ((uint64_t)gridDim.x * 256) >> 6;
    const unsigned lowmask = (1u << M) - 1u;
    for (uint64_t t = wave; t < ntiles; t += nwaves) {
        const uint64_t tile0 = t << (6 + M);
        // lane l: block l of the tile (bi = its GLOBAL index: controls, signs and the populated test may involve shard-id bits)
        const uint64_t bi = B.first + tile0 + ((uint64_t)lane << M);
        unsigned f = (unsigned)(B.basis & lowmask);
        bool pop = (bi & B.fixed_mask) == (B.basis & B.fixed_mask);
        for (unsigned g = 0; g < B.ncam; g++)
            if (((bi >> B.ctl[g]) & 1u) && f < B.C[g]) f = (B.A[g] * f) % B.C[g];
        // one packed word per block for the shuffles: residue | sign << 16, or -1 for an empty block
        const unsigned sgn_blk = (unsigned)__builtin_popcountll(bi & B.sign_mask) & 1u;
        const int code = pop ? (int)(f | (sgn_blk << 16)) : -1;
        const unsigned free_low = (unsigned)(B.hmask & lowmask), sign_low = (unsigned)(B.sign_mask & lowmask);
        const double vp = B.v, vm = -B.v;
        for (unsigned j = 0; j < (1u << M); j++) {
            const unsigned e = j * 64u + lane;                      // element of the tile this lane stores
            const int bc = __shfl(code, (int)(e >> M), 64);        // its block's word
            const unsigned low = e & lowmask;
            amp_t v; v.x = 0.0; v.y = 0.0;
            // with a block structure (ncam > 0, or M bits outside the Hadamard set) the low bits must equal the residue;
            // low bits inside the Hadamard set are free (then ncam == 0 and fixed_mask covers the rest)
            if (bc >= 0 && ((low ^ (unsigned)bc) & ~free_low & lowmask) == 0) {
                const unsigned sg = ((unsigned)bc >> 16) ^ ((unsigned)__builtin_popcount(low & sign_low) & 1u);
                v.x = sg ? vm : vp;
            }
            __builtin_nontemporal_store(v, amp + tile0 + e);
        }
    }
}

// the same rule for M registers beyond the wave tile (M > 12): a workgroup per 2^M-block -- its first wave walks the block's
// residue chain (uniform over the lanes), the whole workgroup writes the block's 2^M amplitudes with coalesced stores
__global__ __launch_bounds__(256) void k_basis_front_big(amp_t *__restrict__ amp, unsigned n, BasisFront B)
{
    __shared__ unsigned s_code[2];
    const unsigned M = B.M;
    const uint64_t nblocks = ((uint64_t)1 << n) >> M;              // host guarantees n >= M
    const unsigned lowmask = (1u << M) - 1u;
    const unsigned free_low = (unsigned)(B.hmask & lowmask), sign_low = (unsigned)(B.sign_mask & lowmask);
    const double vp = B.v, vm = -B.v;
    for (uint64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const uint64_t bi = B.first + (blk << M);                  // GLOBAL index of the block (controls, signs, populated test)
        if (threadIdx.x < 64) {
            unsigned f = (unsigned)(B.basis & lowmask);
            for (unsigned g = 0; g < B.ncam; g++)
                if (((bi >> B.ctl[g]) & 1u) && f < B.C[g]) f = (B.A[g] * f) % B.C[g];
            if (threadIdx.x == 0) {
                s_code[0] = f;
                s_code[1] = ((bi & B.fixed_mask) == (B.basis & B.fixed_mask) ? 2u : 0u) | ((unsigned)__builtin_popcountll(bi & B.sign_mask) & 1u);
            }
        }
        __syncthreads();
        const unsigned f = s_code[0], fl = s_code[1];
        amp_t *to = amp + (blk << M);
        for (unsigned e = threadIdx.x; e <= lowmask; e += 256) {
            amp_t v; v.x = 0.0; v.y = 0.0;
            if ((fl & 2u) && ((e ^ f) & ~free_low & lowmask) == 0) {
                const unsigned sg = (fl & 1u) ^ ((unsigned)__builtin_popcount(e & sign_low) & 1u);
                v.x = sg ? vm : vp;
            }
            __builtin_nontemporal_store(v, to + e);
        }
        __syncthreads();
    }
}

// the circuit front written straight in the COMPACT form of a compact chain ([L register][orbit column], cb column bits): one
// thread per 2^M-block of the real register walks the block's residue chain and writes the block's 2^cb compact amplitudes
// (the one at its residue's place in the orbit = +/- v, the others +0).  B.first = REAL global index of the shard's amplitude 0.
__global__ __launch_bounds__(256) void k_basis_front_compact(amp_t *__restrict__ compact, unsigned n_local_compact, BasisFront B, ExpandParams E)
{
    const unsigned M = B.M, cb = E.cb;
    const uint64_t nblocks = ((uint64_t)1 << n_local_compact) >> cb;
    const unsigned lowmask = (1u << M) - 1u;
    for (uint64_t blk = (uint64_t)blockIdx.x * 256 + threadIdx.x; blk < nblocks; blk += (uint64_t)gridDim.x * 256) {
        const uint64_t bi = B.first + (blk << M);
        unsigned f = (unsigned)(B.basis & lowmask);
        for (unsigned g = 0; g < B.ncam; g++)
            if (((bi >> B.ctl[g]) & 1u) && f < B.C[g]) f = (B.A[g] * f) % B.C[g];
        unsigned col = 0xffu;
        if ((bi & B.fixed_mask) == (B.basis & B.fixed_mask))
            for (unsigned j = 0; j < E.ncols; j++) if (E.orbit[j] == f) col = j;
        const double v = (__builtin_popcountll(bi & B.sign_mask) & 1) ? -B.v : B.v;
        amp_t *to = compact + (blk << cb);
        for (unsigned j = 0; j < (1u << cb); j++) {
            amp_t a; a.x = (j == col) ? v : 0.0; a.y = 0.0;
            to[j] = a;
        }
    }
}

// ---------------------------------------------------------------------------
// X1  local index-bit permutation (pack pass of the sharded qubit remap): dst[j] = src[j with the bit
// pairs (a_m, b_m) exchanged].  Out of place, coalesced stores, gathered loads (runs of 2^min(a, b)).
// ---------------------------------------------------------------------------
struct SwapBits { unsigned npairs; unsigned a[8]; unsigned b[8]; };

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_swap_bits(const amp_t *__restrict__ src, amp_t *__restrict__ dst,
                                                       uint64_t count, SwapBits S)
{
    for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < count; j += (uint64_t)gridDim.x * BLOCK) {
        uint64_t i = j;
        for (unsigned m = 0; m < S.npairs; m++) {
            const uint64_t x = ((i >> S.a[m]) ^ (i >> S.b[m])) & 1u;      // exchange bits a and b
            i ^= (x << S.a[m]) | (x << S.b[m]);
        }
        __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + j);
    }
}

// ---------------------------------------------------------------------------
// X1b  pack + trade in ONE pass, for a sharded register whose shards live in one process (qcx_sharded.inc.h): shard
// `me` of W = 2^k reads its own buffer and writes every amplitude straight into the buffer of the shard that owns it
// after the trade -- peer stores over xGMI when that shard is on another GPU, so the pack pass IS the transfer:
//     j = chunk << zone_lo | low   (chunk = the k trade-zone bits = destination shard)
//     dst[chunk][me << zone_lo | low] = src[j with the bit pairs of S exchanged]
// Blocks are dealt round-robin over the destination shards (block b -> chunk b mod W), so that all W - 1 links of a
// GPU carry traffic at the same time instead of one after the other.  Stores are 1 KiB per wave instruction,
// contiguous in the destination.
// ---------------------------------------------------------------------------
struct PushDst { amp_t *dst[16]; };
// Multi-path striping: with fewer shards than GPUs on the node, the chunk for another shard is cut into
// a direct stripe (blocks [0, nb_direct) of the chunk, stored into the owner's buffer as above) and one stripe per RELAY
// GPU, stored into that GPU's staging area instead (slot = me * W + chunk, `stage_amps` amplitudes each); the host then
// forwards the staged stripes to their owners.  Each stripe rides a different xGMI link out of this GPU.
struct PushRelay { amp_t *stage[8]; unsigned nrelays; uint32_t nb_direct, nb_relay; uint64_t stage_amps; };

template <int BLOCK, bool DEAL>     // DEAL needs BLOCK | 2^zone_lo; small shards take the plain element order
__global__ __launch_bounds__(BLOCK) void k_pack_push(const amp_t *__restrict__ src, PushDst D, PushRelay Rl, uint64_t count, SwapBits S,
                                                       unsigned zone_lo, unsigned klog, unsigned me)
{
    const unsigned W = 1u << klog;
    for (uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; t < count; t += (uint64_t)gridDim.x * BLOCK) {
        unsigned chunk; uint64_t low;
        if (DEAL) { const uint64_t b = t / BLOCK; chunk = (unsigned)(b & (W - 1)); low = (b >> klog) * BLOCK + threadIdx.x; }
        else { chunk = (unsigned)(t >> zone_lo); low = t & (((uint64_t)1 << zone_lo) - 1); }
        uint64_t i = ((uint64_t)chunk << zone_lo) | low;
        for (unsigned m = 0; m < S.npairs; m++) {
            const uint64_t x = ((i >> S.a[m]) ^ (i >> S.b[m])) & 1u;
            i ^= (x << S.a[m]) | (x << S.b[m]);
        }
        amp_t *to = D.dst[chunk] + (((uint64_t)me << zone_lo) | low);
        if (DEAL && Rl.nrelays && chunk != me) {
            const uint64_t lb = low / BLOCK;                            // block of the chunk: uniform over the workgroup
            if (lb >= Rl.nb_direct) {
                unsigned path = (unsigned)((lb - Rl.nb_direct) / Rl.nb_relay);
                if (path >= Rl.nrelays) path = Rl.nrelays - 1;            // (the last relay takes the remainder)
                const uint64_t first = ((uint64_t)Rl.nb_direct + (uint64_t)path * Rl.nb_relay) * BLOCK;
                to = Rl.stage[path] + (uint64_t)(me * W + chunk) * Rl.stage_amps + (low - first);
            }
        }
        __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), to);
    }
}

// ---------------------------------------------------------------------------
// K3b  controlled modular multiply for M registers too large for an LDS tile (M > 12): IN PLACE through a bounded staging
// buffer, a batch of 2^M-blocks at a time.  k_cam_big_gather computes the new rows [0, R) of every control-set block of the
// batch into the staging buffer (R = C in the closed form: rows >= C keep their values; R = 2^M with a source table), with the
// reference's order of summation (ascending source row, starting from 0: Q:393, Q:409-412); k_cam_big_scatter copies them
// back over the block.  No second state buffer and no buffer swap: the path works on a shard view and on a register that fills
// the card.  Traffic: 64 B per rewritten amplitude (gathered read + staged write + staged read + write).
// The 16-B source reads of one block scatter over its 2^M * 16 bytes, so all workgroups that work on a block sit on ONE XCD
// (blockIdx mod 8 under the round-robin placement) and consecutive workgroups of that XCD take consecutive chunks of the same
// block: the block's lines are fetched into that XCD's L2 once (256 KiB at M = 14 ... 2 MiB at M = 17 of the 4 MiB).
// TABLE = false: closed form (control outside the M register, C <= 2^M, no 32-bit wrap);  true: CSR source table.
// ---------------------------------------------------------------------------
struct CamBig {
    unsigned M, R;           // rows staged per block
    int      ctl;            // control bit (>= M), or -1: every block of the view takes part
    unsigned C, d, Cd, inv;
    uint64_t first, nblk;    // the batch: control-set blocks [first, first + nblk) of the view
    unsigned chunks;         // ceil(R / 1024)
};

__device__ __forceinline__ uint64_t cam_big_block_base(const CamBig &P, uint64_t tb)
{
    const uint64_t blockno = (P.ctl >= (int)P.M) ? (insert_zero(tb, (unsigned)P.ctl - P.M) | ((uint64_t)1 << ((unsigned)P.ctl - P.M))) : tb;
    return blockno << P.M;
}

// (block of the batch, chunk of 1024 rows) of workgroup-iteration `it` under the XCD-aware order; false: past the end
__device__ __forceinline__ bool cam_big_item(const CamBig &P, uint64_t it, uint64_t *j, unsigned *chunk)
{
    const unsigned xcd = blockIdx.x & 7u;
    const uint64_t mine = (P.nblk + 7u - xcd) >> 3;               // blocks j of the batch with j mod 8 == xcd
    if (it >= mine * P.chunks) return false;
    *j = (it / P.chunks) * 8u + xcd;
    *chunk = (unsigned)(it % P.chunks);
    return true;
}

template <bool TABLE>
__global__ __launch_bounds__(256) void k_cam_big_gather(const amp_t *__restrict__ amp, amp_t *__restrict__ stage, CamBig P,
                                                        const uint32_t *__restrict__ off, const uint32_t *__restrict__ srcs)
{
    uint64_t j; unsigned chunk;
    for (uint64_t it = blockIdx.x >> 3; cam_big_item(P, it, &j, &chunk); it += gridDim.x >> 3) {
        const amp_t *blk = amp + cam_big_block_base(P, P.first + j);
        amp_t *to = stage + j * P.R;
#pragma unroll
        for (unsigned k = 0; k < 4; k++) {
            const unsigned g = chunk * 1024u + k * 256u + threadIdx.x;
            if (g >= P.R) continue;
            amp_t acc; acc.x = 0.0; acc.y = 0.0;
            if (TABLE) {
                for (uint32_t s = off[g]; s < off[g + 1]; s++) { const amp_t v = blk[srcs[s]]; acc.x += v.x; acc.y += v.y; }
            } else if (g % P.d == 0) {
                uint32_t s0 = (uint32_t)(((uint64_t)(g / P.d) * P.inv) % P.Cd);
                for (uint32_t q = 0; q < P.d; q++, s0 += P.Cd) { const amp_t v = blk[s0]; acc.x += v.x; acc.y += v.y; }
            }
            __builtin_nontemporal_store(acc, to + g);
        }
    }
}

__global__ __launch_bounds__(256) void k_cam_big_scatter(amp_t *__restrict__ amp, const amp_t *__restrict__ stage, CamBig P)
{
    uint64_t j; unsigned chunk;
    for (uint64_t it = blockIdx.x >> 3; cam_big_item(P, it, &j, &chunk); it += gridDim.x >> 3) {
        amp_t *blk = amp + cam_big_block_base(P, P.first + j);
        const amp_t *from = stage + j * P.R;
        amp_t v[4];
#pragma unroll
        for (unsigned k = 0; k < 4; k++) {
            const unsigned g = chunk * 1024u + k * 256u + threadIdx.x;
            if (g < P.R) v[k] = __builtin_nontemporal_load(from + g);
        }
#pragma unroll
        for (unsigned k = 0; k < 4; k++) {
            const unsigned g = chunk * 1024u + k * 256u + threadIdx.x;
            if (g < P.R) blk[g] = v[k];
        }
    }
}

// ---------------------------------------------------------------------------
// K10  marginal probabilities of a contiguous qubit range (qcx_marginal_probabilities, DESIGN s4.5d).  probs[v] = the PAIRWISE
// TREE, over the summed bits (every bit outside the range) in ascending order, of p_i = fl(fl(re*re) + fl(im*im)): level h adds
// the pairs of partial sums that differ only in the h-th lowest summed bit.  The planner (qcx_api.hip, marginal_plan) cuts the
// tree into stages; a stage reduces the lowest summed bits that are left, inside TILES of 2^T elements of its input array (the
// c lowest index bits -- whole 128-B runs -- plus summed bits above them, then kept bits to fill the tile), and writes the
// partial sums indexed by its input's remaining bits in ascending order.  Every summed bit below a tile's highest summed bit
// lies inside the tile, so the in-tile tree is a prefix of the whole tree, and the stages compose to exactly that tree.
//   MARG_AMP      the stage reads amplitudes (leaf = |a|^2, no FMA)
//   MARG_DBL      the stage reads the double partials of the stage before
//   MARG_COMPACT  the stage reads a circuit's compact result in place: element = one L-register block, whose 2^M-leaf tree has
//                 +0 leaves everywhere except at the orbit residues (x + 0 = x: the sparse tree P.prog is the same bits); a
//                 padding column that is not +0 sets *P.bad (the caller then falls back to the expanded register)
// Nothing is written but the stage's output (and *P.bad).
// ---------------------------------------------------------------------------
enum { MARG_AMP = 0, MARG_DBL = 1, MARG_COMPACT = 2 };
struct MargSeg { uint8_t src, dst_in, dst_out, len; };
struct MargParams {
    const void *src;
    double *dst;
    unsigned *bad;                  // MARG_COMPACT: set to 1 when a padding column holds anything but +0
    uint64_t ntiles;
    uint32_t T, nlvl, nkeep, nseg;
    uint8_t tpos[16];               // input index bit of tile-local bit j
    uint8_t lvl_q[16];              // level h sums the partials that differ in bit lvl_q[h] of the compacted tile index
    uint8_t kpos[16];               // output index bit of the i-th bit left in the tile (ascending)
    MargSeg seg[40];                // tile number bits [src, src + len) -> input bits dst_in.. / output bits dst_out..
    uint32_t cb, ncols, nprog;      // MARG_COMPACT: 2^cb columns per block, the first ncols hold the orbit; the sparse tree:
    uint8_t prog_a[16], prog_b[16]; //   slot[prog_a[k]] += slot[prog_b[k]], k < nprog (slot j = column j; the root is slot 0)
};

template <int KIND>
__global__ __launch_bounds__(256) void k_marginal(MargParams P)
{
    // a thread loads 16 elements of the tile (MARG_COMPACT: 16 amplitudes of its 2^8 blocks, 2^cb <= 16 columns each, in
    // index order: a wave reads whole runs of blocks)
    constexpr unsigned EPT = 16u;
    constexpr unsigned CROW = 17u;                                   // (padded row of a block's columns: fewer bank conflicts)
    __shared__ double buf[KIND == MARG_COMPACT ? 256u * (CROW + 1u) : 4096u];
    // the parameters indexed at run time, in LDS: read from the kernel arguments they would be vector loads, and every wait for
    // one of them would also wait for the next tile's amplitude loads in flight
    __shared__ uint8_t s_tpos[16], s_lvlq[16], s_kpos[16];
    __shared__ MargSeg s_seg[40];
    double *red = KIND == MARG_COMPACT ? buf + 256u * CROW : buf;
    const unsigned tid = threadIdx.x, nel = 1u << P.T;
    const unsigned cb = KIND == MARG_COMPACT ? P.cb : 0u, ncb = 1u << cb;
    if (tid < 16) { s_tpos[tid] = P.tpos[tid]; s_lvlq[tid] = P.lvl_q[tid]; s_kpos[tid] = P.kpos[tid]; }
    if (tid < 40) s_seg[tid] = P.seg[tid];
    __syncthreads();
    // element j of this thread: tile-local element e = (tid + 256 j) >> cb, column (tid + 256 j) mod 2^cb; off[j] = its offset
    uint64_t off[EPT];
    unsigned nld = 0;                                                // elements this thread loads (the first nld j)
#pragma unroll
    for (unsigned j = 0; j < EPT; j++) {
        const unsigned i = tid + 256u * j, e = i >> cb;
        uint64_t o = 0;
        for (unsigned b = 0; b < P.T; b++) o |= (uint64_t)((e >> b) & 1u) << s_tpos[b];
        off[j] = (o << cb) | (i & (ncb - 1u));
        if (e < nel && (KIND != MARG_COMPACT || j < ncb)) nld = j + 1;
    }
    auto base_of = [&](uint64_t t, bool out) {
        uint64_t b = 0;
        for (unsigned s = 0; s < P.nseg; s++)
            b |= ((t >> s_seg[s].src) & ((((uint64_t)1) << s_seg[s].len) - 1u)) << (out ? s_seg[s].dst_out : s_seg[s].dst_in);
        return b;
    };
    // the next tile's loads are issued before this tile's tree levels run (they are in flight meanwhile); a whole tile of loads
    // without a guard, so that each use waits for its own load only
    typedef typename std::conditional<KIND == MARG_DBL, double, amp_t>::type ld_t;
    ld_t a[EPT];
    const bool full = nld == EPT;
    auto load = [&](uint64_t t) {
        const uint64_t base = base_of(t, false) << cb;
        if (full) {
#pragma unroll
            for (unsigned j = 0; j < EPT; j++) {
                if constexpr (KIND == MARG_DBL) a[j] = ((const double *)P.src)[base | off[j]];
                else a[j] = __builtin_nontemporal_load((const amp_t *)P.src + (base | off[j]));
            }
        } else {
#pragma unroll
            for (unsigned j = 0; j < EPT; j++)
                if (j < nld) {
                    if constexpr (KIND == MARG_DBL) a[j] = ((const double *)P.src)[base | off[j]];
                    else a[j] = __builtin_nontemporal_load((const amp_t *)P.src + (base | off[j]));
                }
        }
    };
    auto leaf = [&](unsigned j) {
        if constexpr (KIND == MARG_DBL) return a[j];
        else return a[j].x * a[j].x + a[j].y * a[j].y;
    };
    if (blockIdx.x < P.ntiles) load(blockIdx.x);
    for (uint64_t t = blockIdx.x; t < P.ntiles; t += gridDim.x) {
        const uint64_t base_out = base_of(t, true);
        if constexpr (KIND != MARG_COMPACT) {
            if (full) {
#pragma unroll
                for (unsigned j = 0; j < EPT; j++) red[tid + 256u * j] = leaf(j);
            } else {
#pragma unroll
                for (unsigned j = 0; j < EPT; j++)
                    if (j < nld) red[tid + 256u * j] = leaf(j);
            }
            if (t + gridDim.x < P.ntiles) load(t + gridDim.x);
        } else {
            // the leaves of block e's orbit columns into its LDS row; a padding column must hold +0
            bool bad = false;
#pragma unroll
            for (unsigned j = 0; j < EPT; j++)
                if (j < nld) {
                    const unsigned i = tid + 256u * j, e = i >> cb, col = i & (ncb - 1u);
                    if (col < P.ncols) buf[e * CROW + col] = leaf(j);
                    else bad |= (__double_as_longlong(a[j].x) | __double_as_longlong(a[j].y)) != 0;
                }
            if (bad) *P.bad = 1u;                                    // (a plain store: every writer stores the same value)
            if (t + gridDim.x < P.ntiles) load(t + gridDim.x);
            __syncthreads();
            // each block's sparse tree over its 2^M leaves (+0 but at the orbit residues)
            if (tid < nel) {
                double *row = buf + tid * CROW;
                for (unsigned k = 0; k < P.nprog; k++) row[P.prog_a[k]] = row[P.prog_a[k]] + row[P.prog_b[k]];
                red[tid] = row[0];
            }
        }
        __syncthreads();
        // the tree levels inside the tile, lowest summed bit first; in place (read all, barrier, write all)
        unsigned sz = nel;
        for (unsigned h = 0; h < P.nlvl; h++) {
            const unsigned half = sz >> 1, q = s_lvlq[h], lo = (1u << q) - 1u;
            double v[EPT > 8 ? 8 : 1];
#pragma unroll
            for (unsigned m = 0; m < (EPT > 8 ? 8u : 1u); m++) {
                const unsigned k = tid + 256u * m;
                if (k < half) {
                    const unsigned i0 = ((k & ~lo) << 1) | (k & lo);
                    v[m] = red[i0] + red[i0 | (1u << q)];
                }
            }
            __syncthreads();
#pragma unroll
            for (unsigned m = 0; m < (EPT > 8 ? 8u : 1u); m++) {
                const unsigned k = tid + 256u * m;
                if (k < half) red[k] = v[m];
            }
            __syncthreads();
            sz = half;
        }
        for (unsigned k = tid; k < sz; k += 256u) {
            uint64_t o = base_out;
            for (unsigned b = 0; b < P.nkeep; b++) o |= (uint64_t)((k >> b) & 1u) << s_kpos[b];
            P.dst[o] = red[k];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// The tiling K14 and K15 walk a Pauli string (x_mask, z_mask) with.  A tile is the 2^T lowest index bits, T = min(n, 12); a
// workgroup of 256 threads owns one, thread element j = tile-local e = tid + 256 j, j < EPT (n < 12: one partial tile, the
// first nld elements of a thread exist).  The partner of index i is i ^ x_mask: element e ^ x_low of tile t ^ xh.
//   PAIR (xh != 0): a unit of work is the pair of tiles (t, t ^ xh), t the one with the highest set bit hb of xh clear:
//        tile_of(u) puts a zero into u at that bit.  Otherwise a unit is a tile.
//   e ^ x_low = (tid ^ x_low's 8 low bits) + 256 (j ^ x_low's bits above): one lane offset (partner_lane), uniform steps
//        (partner_elem), whole 128-B lines either way.
//   popcount(i & z_mask) mod 2 = par(tile) + bit j of sodd (the thread's own element e) or of podd (its partner's e ^ x_low)
// ---------------------------------------------------------------------------
template <bool PAIR>
struct PauliTiles {
    static constexpr unsigned EPT = 16u;
    unsigned T, nel, x_low, z_low, hb, nld, podd, sodd;
    uint64_t xh, zh;
    __device__ __forceinline__ PauliTiles(unsigned T_, uint64_t x_mask, uint64_t z_mask, unsigned tid)
        : T(T_), nel(1u << T_), x_low((unsigned)x_mask & (nel - 1u)), z_low((unsigned)z_mask & (nel - 1u)),
          hb(PAIR ? 63u - (unsigned)__clzll((long long)(x_mask >> T_)) : 0u), nld(0), podd(0), sodd(0),
          xh(x_mask >> T_), zh(z_mask >> T_)
    {
#pragma unroll
        for (unsigned j = 0; j < EPT; j++) {
            const unsigned e = tid + 256u * j;
            if (e < nel) nld = j + 1;
            podd |= (unsigned)(__popc((e ^ x_low) & z_low) & 1) << j;
            sodd |= (unsigned)(__popc(e & z_low) & 1) << j;
        }
    }
    __device__ __forceinline__ uint64_t tile_of(uint64_t u) const
    {
        if constexpr (PAIR) return ((u >> hb) << (hb + 1u)) | (u & ((((uint64_t)1) << hb) - 1u));
        else return u;
    }
    __device__ __forceinline__ unsigned par(uint64_t tile) const { return (unsigned)__popcll(tile & zh); }
    __device__ __forceinline__ unsigned partner_lane(unsigned tid) const { return tid ^ (x_low & 255u); }
    __device__ __forceinline__ unsigned partner_elem(unsigned j) const { return j ^ (x_low >> 8); }
};

// ---------------------------------------------------------------------------
// K14  the first stage of a Pauli string's expectation value (qcx_pauli_expectation, DESIGN s4.5h; tests/pauli_ref.py is the
// definition).  The string is (x_mask, z_mask), Y on x_mask & z_mask, g = popcount(x_mask & z_mask) mod 4.  The leaf of index i,
// with a = amp[i] and b = amp[i ^ x_mask], every product and sum rounded on its own (no FMA):
//     t = g even ? a.re * b.re + a.im * b.im : a.im * b.re - a.re * b.im
//     leaf_i = 0.0 + (odd ? -t : t),   odd = (popcount((i ^ x_mask) & z_mask) + (g >> 1)) & 1
// (the "0.0 +" turns a -0 into +0 and nothing else), and the value is K10's pairwise tree over all index bits on these leaves.
// This kernel is stage 0 of qcx_marginal_plan(n, 0, 0): PauliTiles' tiles (T = min(n, 12) lowest index bits), all of them summed, so
// tile t's root goes to dst[t] and the later stages are plain k_marginal<MARG_DBL> launches.  Loads, the next unit's loads in
// flight during the tree levels, and the levels themselves are k_marginal<MARG_AMP>'s.  Sign and g come from the index and the
// arguments: no table.  A unit of work is
//   SHAPE 0  a tile, x_mask == 0: b is a itself
//   SHAPE 1  a tile, the partner inside it (x_mask < 2^T): the tile's amplitudes go through LDS once (64 KiB, the leaves then
//            take the same space), a thread reads a at e and b at e ^ x_mask back from there
//   SHAPE 2  the PAIR of tiles (t, t ^ xh) (PauliTiles): a from tile t at e, b from the partner tile at e ^ x_low.  leaf_i and
//            leaf_(i ^ x_mask) are the same bits (products commute; a difference taken the other way round is negated
//            exactly, and the sign flips with it), so each leaf is computed ONCE and placed at e of t's tree and at
//            e ^ x_low of the partner's.  The two trees
//            lie behind each other in LDS (2 x 32 KiB) and reduce as one array of 2^13: a level's pairs never straddle them.
//            Every amplitude comes from HBM once, for any string.
// FULL: the tile has all 2^12 elements (n >= 12) and nothing in the unit's path is guarded -- a guard around a load makes every
// wait a wait for all loads, the prefetched ones included; !FULL is the one partial tile of a register below 12 qubits.
// Nothing is written but dst.
// ---------------------------------------------------------------------------
template <int SHAPE, bool FULL>
__global__ __launch_bounds__(256) void k_pauli_leaves(const amp_t *__restrict__ amp, double *__restrict__ dst, uint64_t nunits,
                                                      unsigned T, uint64_t x_mask, uint64_t z_mask, unsigned g)
{
    using Tiles = PauliTiles<SHAPE == 2>;
    constexpr unsigned EPT = Tiles::EPT;
    constexpr unsigned NRED = SHAPE == 0 ? 4096u : 8192u;
    constexpr unsigned VPT = SHAPE == 2 ? 16u : 8u;                  // sums a thread forms at the widest tree level
    __shared__ double red[NRED];
    const unsigned tid = threadIdx.x;
    const Tiles P(T, x_mask, z_mask, tid);
    const unsigned nel = P.nel, x_low = P.x_low, nld = P.nld;
    const uint64_t xh = P.xh;
    const bool godd = (g & 1u) != 0;
    amp_t a[EPT], b[SHAPE == 2 ? EPT : 1];
    auto load = [&](uint64_t u) {
        const uint64_t t = P.tile_of(u);
        const amp_t *pa = amp + (t << T) + tid;
#pragma unroll
        for (unsigned j = 0; j < EPT; j++)
            if (FULL || j < nld) a[j] = __builtin_nontemporal_load(pa + 256u * j);
        if constexpr (SHAPE == 2) {
            const amp_t *pb = amp + ((t ^ xh) << T) + P.partner_lane(tid);
#pragma unroll
            for (unsigned j = 0; j < EPT; j++) b[j] = __builtin_nontemporal_load(pb + 256u * P.partner_elem(j));
        }
    };
    auto leaf = [&](amp_t p, amp_t q, unsigned j, unsigned tile_par) {
        // g even: p.re q.re + p.im q.im; g odd: p.im q.re - p.re q.im = p.im q.re + (-(p.re q.im)), the same rounding; no branch
        const double u = (godd ? p.y : p.x) * q.x, w = (godd ? p.x : p.y) * q.y;
        const double t = u + (godd ? -w : w);
        return 0.0 + (((tile_par + (P.podd >> j)) & 1u) ? -t : t);
    };
    if (blockIdx.x < nunits) load(blockIdx.x);
    for (uint64_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const uint64_t t = P.tile_of(u);
        const unsigned tile_par = P.par(t ^ xh) + (g >> 1);
        if constexpr (SHAPE == 1) {
            // through LDS: once the tile is there, a's registers are free for the next tile's loads, which go out at once;
            // a thread then reads e and e ^ x_low back, keeps its leaves, and writes them when all have read
            amp_t *sa = (amp_t *)red;
#pragma unroll
            for (unsigned j = 0; j < EPT; j++)
                if (FULL || j < nld) sa[tid + 256u * j] = a[j];
            __syncthreads();
            if (u + gridDim.x < nunits) load(u + gridDim.x);
            double v[EPT];
#pragma unroll
            for (unsigned j = 0; j < EPT; j++)
                if (FULL || j < nld) v[j] = leaf(sa[tid + 256u * j], sa[(tid + 256u * j) ^ x_low], j, tile_par);
            __syncthreads();
#pragma unroll
            for (unsigned j = 0; j < EPT; j++)
                if (FULL || j < nld) red[tid + 256u * j] = v[j];
        } else {
#pragma unroll
            for (unsigned j = 0; j < EPT; j++)
                if (FULL || j < nld) {
                    const double v = leaf(a[j], SHAPE == 2 ? b[SHAPE == 2 ? j : 0] : a[j], j, tile_par);
                    red[tid + 256u * j] = v;
                    if constexpr (SHAPE == 2) red[4096u + ((tid + 256u * j) ^ x_low)] = v;
                }
            if (u + gridDim.x < nunits) load(u + gridDim.x);
        }
        __syncthreads();
        // the tree levels inside the tile, lowest bit first; in place (read all, barrier, write all)
        unsigned sz = SHAPE == 2 ? 2u * nel : nel;
        for (unsigned h = 0; h < T; h++) {
            const unsigned half = sz >> 1;
            double v[VPT];
#pragma unroll
            for (unsigned m = 0; m < VPT; m++) {
                const unsigned k = tid + 256u * m;
                if (k < half) v[m] = red[2u * k] + red[2u * k + 1u];
            }
            __syncthreads();
#pragma unroll
            for (unsigned m = 0; m < VPT; m++) {
                const unsigned k = tid + 256u * m;
                if (k < half) red[k] = v[m];
            }
            __syncthreads();
            sz = half;
        }
        if (tid == 0) dst[t] = red[0];
        if (SHAPE == 2 && tid == 1) dst[t ^ xh] = red[1];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// K14b  K14's stage 0 for K <= QCX_PAULI_BATCH_W strings that SHARE their x_mask, from one read of the state
// (qcx_pauli_expectation_batch, DESIGN s4.5h).  What depends on x_mask alone -- the operands a = amp[i], b = amp[i ^ x_mask] and
// the two candidate sums t_even = a.re b.re + a.im b.im, t_odd = a.im b.re - a.re b.im -- is formed once per tile and kept in
// registers (ODD: some term of the pass has odd g; otherwise t_odd is never formed); a term then only picks one of the two
// (kernel-uniform), puts its signs on and reduces the tile's tree.  Units, shapes, FULL and the loads are K14's.
// The tree is K14's tree, level h adding the partial sums that differ in bit h of the tile-local e, but no term has a tree in
// LDS.  ONCE per tile the t values change hands through LDS so that a thread holds 16 CONSECUTIVE elements, e = 16 tid + i
// (in the exchange shape the amplitudes already go through LDS, as in K14: a thread reads a and b back in that layout and forms
// t there).  Per term, then:
//   bits 0-3 (i)          15 sums in the thread, lowest bit first
//   bits 4-9 (the lane)   six butterfly levels on ONE value (IEEE addition commutes: both lanes of a pair form the same sum)
//   bits 10-11 (the wave) one double per wave and term through LDS (wsum); ONE barrier per tile serves all terms, and thread k
//                         forms (w0 + w1) + (w2 + w3) of term k
// Rows of 16 elements lie 16 B apart in LDS, so that the 128-bit reads of a row hit all banks.
// Three facts about the arithmetic make this K14's bits (tests/test_pauli_batch_plan.py checks them against the definition):
//   - in the pair shape the partner tile's tree holds the same leaves at e ^ x_low, so every level adds the same two numbers
//     (perhaps the other way round) and its root is tile t's root: one tree, written to both partials
//   - a leaf's "0.0 +" may wait until the root: with signed-zero leaves a node differs from the canonical tree only where it is
//     a zero of the other sign, and 0.0 + root is then the same +0
//   - for the same reason the leaves a partial tile (n < 12) does not have are zeros of either sign: the levels above T add
//     zeros to the T-level root.
// The sign of term k on element i: par((e ^ x_low) & z_low) = par((tid ^ (x_low >> 4)) & (z_low >> 4)) + bit i of the term's
// iodd (the same for every thread: the host computes it), + par((tile ^ xh) & zh) + (g >> 1), scalar.  Terms come as a kernel
// argument.  Term k's root of tile t goes to dst[k * row_stride + t].  Nothing is written but dst.
// ---------------------------------------------------------------------------
#define QCX_PAULI_BATCH_W 32
struct PauliBatchTerms {
    uint64_t z[QCX_PAULI_BATCH_W];
    uint32_t meta[QCX_PAULI_BATCH_W];            // iodd (bit i: par((i ^ (x_low & 15)) & (z_low & 15))) | g << 16
};

template <int CTRL> __device__ __forceinline__ double pauli_dpp(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
constexpr int PAULI_DPP_XOR1 = 0xB1, PAULI_DPP_XOR2 = 0x4E;       // quad_perm [1, 0, 3, 2] and [2, 3, 0, 1]

template <int SHAPE, bool FULL, bool ODD>
__global__ __launch_bounds__(256) void k_pauli_leaves_batch(const amp_t *__restrict__ amp, double *__restrict__ dst, uint64_t row_stride,
                                                            uint64_t nunits, unsigned T, uint64_t x_mask, unsigned K, PauliBatchTerms terms)
{
    using Tiles = PauliTiles<SHAPE == 2>;
    constexpr unsigned EPT = Tiles::EPT;
    static_assert(EPT == 16, "a thread's elements are one row of 16");
    // a tile in LDS, 16 B of padding behind every row of 16: its amplitudes (the exchange shape), or else its t values
    constexpr unsigned AMPS = 256u * 17u, TVAL2 = 256u * 9u;         // in amplitudes, and in pairs of doubles
    __shared__ __attribute__((aligned(16))) double lds[SHAPE == 1 ? 2u * AMPS : (ODD ? 4u : 2u) * TVAL2];
    __shared__ double wsum[QCX_PAULI_BATCH_W * 4];                   // [term][wave]
    const unsigned tid = threadIdx.x, wave = tid >> 6;
    const Tiles P(T, x_mask, 0, tid);
    const unsigned nel = P.nel, x_low = P.x_low, nld = P.nld;
    const uint64_t xh = P.xh;
    auto amp_pos = [](unsigned e) { return e + (e >> 4); };
    amp_t a[EPT], b[SHAPE == 2 ? EPT : 1];
    auto load = [&](uint64_t u) {
        const uint64_t t = P.tile_of(u);
        const amp_t *pa = amp + (t << T) + tid;
#pragma unroll
        for (unsigned j = 0; j < EPT; j++)
            if (FULL || j < nld) a[j] = __builtin_nontemporal_load(pa + 256u * j);
        if constexpr (SHAPE == 2) {
            const amp_t *pb = amp + ((t ^ xh) << T) + P.partner_lane(tid);
#pragma unroll
            for (unsigned j = 0; j < EPT; j++) b[j] = __builtin_nontemporal_load(pb + 256u * P.partner_elem(j));
        }
    };
    auto t_even = [](amp_t p, amp_t q) { return p.x * q.x + p.y * q.y; };
    auto t_odd = [](amp_t p, amp_t q) { return p.y * q.x - p.x * q.y; };
    // term k on the thread's row of t values: signs, the tree's levels up to the wave, the wave's sum into wsum
    auto reduce = [&](const double (&tv)[EPT], unsigned k, unsigned flip, unsigned iodd) {
        double v[EPT];
#pragma unroll
        for (unsigned i = 0; i < EPT; i++)
            v[i] = __hiloint2double(__double2hiint(tv[i]) ^ (int)(flip ^ (((iodd >> i) & 1u) << 31)), __double2loint(tv[i]));
#pragma unroll
        for (unsigned i = 0; i < 8u; i++) v[i] = v[2u * i] + v[2u * i + 1u];
#pragma unroll
        for (unsigned i = 0; i < 4u; i++) v[i] = v[2u * i] + v[2u * i + 1u];
        double s = (v[0] + v[1]) + (v[2] + v[3]);
        s = s + pauli_dpp<PAULI_DPP_XOR1>(s);
        s = s + pauli_dpp<PAULI_DPP_XOR2>(s);
        s = s + __shfl_xor(s, 4);
        s = s + __shfl_xor(s, 8);
        s = s + __shfl_xor(s, 16);
        s = s + __shfl_xor(s, 32);
        if ((tid & 63u) == 0) wsum[k * 4u + wave] = s;
    };
    if (blockIdx.x < nunits) load(blockIdx.x);
    for (uint64_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const uint64_t t = P.tile_of(u);
        double te[EPT], to[ODD ? EPT : 1];
        if constexpr (SHAPE == 1) {
            // as K14: once the tile is in LDS, a's registers take the next tile's loads; a thread reads its row and the partners'
            amp_t *sa = (amp_t *)lds;
#pragma unroll
            for (unsigned j = 0; j < EPT; j++)
                if (FULL || j < nld) sa[amp_pos(tid + 256u * j)] = a[j];
            __syncthreads();
            if (u + gridDim.x < nunits) load(u + gridDim.x);
#pragma unroll
            for (unsigned i = 0; i < EPT; i++) {
                const unsigned e = 16u * tid + i;
                if (FULL || e < nel) {
                    const amp_t p = sa[amp_pos(e)], q = sa[amp_pos(e ^ x_low)];
                    te[i] = t_even(p, q);
                    if constexpr (ODD) to[i] = t_odd(p, q);
                } else { te[i] = 0.0; if constexpr (ODD) to[i] = 0.0; }
            }
        } else {
            double2 *se = (double2 *)lds, *so = (double2 *)lds + TVAL2;
#pragma unroll
            for (unsigned j = 0; j < EPT; j++)
                if (FULL || j < nld) {
                    const unsigned e = tid + 256u * j;
                    const amp_t q = SHAPE == 2 ? b[SHAPE == 2 ? j : 0] : a[j];
                    ((double *)(se + (e >> 4) * 9u))[e & 15u] = t_even(a[j], q);
                    if constexpr (ODD) ((double *)(so + (e >> 4) * 9u))[e & 15u] = t_odd(a[j], q);
                }
            __syncthreads();
            if (u + gridDim.x < nunits) load(u + gridDim.x);
#pragma unroll
            for (unsigned i = 0; i < EPT; i += 2) {
                const bool there = FULL || 16u * tid + i < nel;      // (nel is even: the two are there together)
                const double2 ve = se[tid * 9u + (i >> 1)];
                te[i] = there ? ve.x : 0.0;
                te[i + 1] = there ? ve.y : 0.0;
                if constexpr (ODD) {
                    const double2 vo = so[tid * 9u + (i >> 1)];
                    to[i] = there ? vo.x : 0.0;
                    to[i + 1] = there ? vo.y : 0.0;
                }
            }
        }
        for (unsigned k = 0; k < K; k++) {
            const uint64_t z = terms.z[k];
            const unsigned meta = terms.meta[k], g = meta >> 16, z_low = (unsigned)z & (nel - 1u);
            const unsigned odd = (unsigned)__popc((tid ^ (x_low >> 4)) & (z_low >> 4)) + (unsigned)__popcll((t ^ xh) & (z >> T)) + (g >> 1);
            if constexpr (ODD) {
                if (g & 1u) reduce(to, k, odd << 31, meta & 0xFFFFu);
                else reduce(te, k, odd << 31, meta & 0xFFFFu);
            } else
                reduce(te, k, odd << 31, meta & 0xFFFFu);
        }
        __syncthreads();
        if (tid < K) {
            const double *w = wsum + 4u * tid;
            const double root = 0.0 + ((w[0] + w[1]) + (w[2] + w[3]));
            dst[tid * row_stride + t] = root;
            if constexpr (SHAPE == 2) dst[tid * row_stride + (t ^ xh)] = root;
        }
        // (the next tile writes lds, which all have read before the barrier above, and wsum only behind its own first barrier)
    }
}

// ---------------------------------------------------------------------------
// K11  collapse of the qubit range [first, first + num) onto `outcome` (qcx_measure_qubits, DESIGN s4.5e).  An amplitude whose
// range bits equal `outcome` becomes (fl(re * s), fl(im * s)) -- two products, nothing to contract into an FMA --, every other
// one (+0, +0) and is NEVER READ: its lane only stores.  A wave takes 64 amplitudes per step, lane l the element e = 64 t + l of
// wave-tile t; a workgroup takes 256 U consecutive elements a step, U per lane (all U loads are issued before the first store).
//   PERM = false: index = e.  Kept-or-dropped is the same for a whole wave when first >= 6 (and lines are mixed when first < 3:
//                 a lane's load is predicated, the line comes in whole either way).
//   PERM = true (3 <= first < 6, n >= num + 6): the 6 - first lane bits that would fall into the range are moved ABOVE it, the
//                 range takes tile-number bits instead: index = e[0, first) | e[6, 6 + num) << first | e[first, 6) << (first + num)
//                 | e[6 + num, ..) << (6 + num).  A wave instruction then covers 2^(6 - first) runs of 2^first amplitudes (whole
//                 128-B lines) that share their range bits: the branch is wave-uniform again.
// ---------------------------------------------------------------------------
template <bool PERM, int U>
__global__ __launch_bounds__(256) void k_collapse_range(amp_t *__restrict__ amp, uint64_t count, unsigned first, unsigned num,
                                                        uint64_t outcome, double s)
{
    const uint64_t rmask = ((uint64_t)1 << num) - 1u;
    const uint64_t lowmask = ((uint64_t)1 << first) - 1u;
    for (uint64_t e0 = (uint64_t)blockIdx.x * (256u * U) + threadIdx.x; e0 < count; e0 += (uint64_t)gridDim.x * (256u * U)) {
        uint64_t idx[U];
        bool keep[U];
        amp_t v[U];
#pragma unroll
        for (unsigned u = 0; u < (unsigned)U; u++) {
            const uint64_t e = e0 + u * 256u;
            uint64_t i = e;
            if (PERM) {
                const uint64_t up = e >> 6;                                  // tile number: range bits, then the bits above the moved ones
                i = (e & lowmask) | ((up & rmask) << first) | (((e & 63u) >> first) << (first + num)) | ((up >> num) << (6u + num));
            }
            idx[u] = i;
            keep[u] = e < count && ((i >> first) & rmask) == outcome;
            v[u].x = 0.0; v[u].y = 0.0;
            if (keep[u]) v[u] = __builtin_nontemporal_load(amp + i);
        }
#pragma unroll
        for (unsigned u = 0; u < (unsigned)U; u++) {
            if (keep[u]) { v[u].x = v[u].x * s; v[u].y = v[u].y * s; }
            if (e0 + u * 256u < count) __builtin_nontemporal_store(v[u], amp + idx[u]);
        }
    }
}

// ---------------------------------------------------------------------------
// K12  any one-qubit gate, plain or controlled (qcx_one_qubit_gate / qcx_c_one_qubit_gate, DESIGN s4.5f): the 2x2 matrix
// u = (u00 u01; u10 u11) on the pairs (i0, i1 = i0 | 2^q), as the reference's mat-vec would apply it from four stored
// triplets per pair taken in column order (Q:396-413; the construction of Q:456-481 / Q:529-562 with free entries):
//     lo = q_row(u00 * a, u01 * b),   hi = q_row(u10 * a, u11 * b),    products by q_mul (the pinned arithmetic: see there),
// all four entries multiplied out even where they are zero.  The eight components are kernel arguments (SGPRs); no LDS, no
// table, one arithmetic path for every matrix.
// The kernels are k_h_pair / k_h_wave / k_phase / k_phase_lines with this butterfly in place of theirs.  A result is never
// -0 (the second addend meets a first sum that is not -0), so the invariant of K0c holds behind them.
// ---------------------------------------------------------------------------
struct UMat { double r00, i00, r01, i01, r10, i10, r11, i11; };

// one row; a = the pair's amplitude with the target bit clear, b = with it set
__device__ __forceinline__ amp_t u_row(double m0r, double m0i, double m1r, double m1i, amp_t a, amp_t b)
{
    return q_row(q_mul(m0r, m0i, a), q_mul(m1r, m1i, b));          // columns i0 then i1
}

__device__ __forceinline__ void u_butterfly(const UMat &U, amp_t &a, amp_t &b)
{
    const amp_t lo = u_row(U.r00, U.i00, U.r01, U.i01, a, b);
    const amp_t hi = u_row(U.r10, U.i10, U.r11, U.i11, a, b);
    a = lo; b = hi;
}

// K12a  pair form, any target qubit (k_h_pair's shape).  CTL: only the pairs whose control bit c is set are read and
// written -- c is a second squeezed-out index bit (as in k_phase<NB>), npairs = 2^(n-2).  PPT pairs per lane are loaded
// before any is stored; stream-interleaved tile order as in k_phase.
template <int PPT, bool NT, bool CTL, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_u_pair(amp_t *__restrict__ amp, unsigned q, unsigned c, UMat U, uint64_t npairs,
                                                    unsigned glog, unsigned slog)
{
    const uint64_t bit = (uint64_t)1 << q, cbit = (uint64_t)1 << c;
    const unsigned b0 = (CTL && c < q) ? c : q, b1 = (c < q) ? q : c;      // the squeezed-out bits, ascending
    const uint64_t step = (uint64_t)gridDim.x * (BLOCK * PPT);
    const uint64_t tile0 = stream_tile(glog, slog);
    for (uint64_t base = tile0 * (BLOCK * PPT); base < npairs; base += step) {
        amp_t a[PPT], b[PPT];
        uint64_t i0[PPT];
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            const uint64_t p = base + (uint64_t)k * BLOCK + threadIdx.x;
            uint64_t i = insert_zero(p, b0);
            if (CTL) i = insert_zero(i, b1) | cbit;
            i0[k] = i;
            if (p < npairs) { a[k] = ld<NT>(amp + i); b[k] = ld<NT>(amp + i + bit); }
        }
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            const uint64_t p = base + (uint64_t)k * BLOCK + threadIdx.x;
            if (p < npairs) {
                u_butterfly(U, a[k], b[k]);
                st<NT>(amp + i0[k], a[k]);
                st<NT>(amp + i0[k] + bit, b[k]);
            }
        }
    }
}

// K12b  wave-tile form for low targets (k_h_wave's shape: 64 * R consecutive amplitudes as R registers x 64 lanes).
// Q < 6: the partner arrives by xor-shuffle and every lane computes its OWN row -- the lower lane (0 + u00 * own) + u01 * other,
// the upper lane (0 + u10 * other) + u11 * own: the column order of the definition, the partner's product first up there.
// Q >= 6: the partner is another register of the same lane.
template <int Q, int R>
__device__ __forceinline__ void u_wave_tile(const UMat &U, amp_t (&r)[R], unsigned lane)
{
    if constexpr (Q < 6) {
        const bool upper = (lane >> Q) & 1u;
        const double m0r = upper ? U.r10 : U.r00, m0i = upper ? U.i10 : U.i00;
        const double m1r = upper ? U.r11 : U.r01, m1i = upper ? U.i11 : U.i01;
#pragma unroll
        for (int k = 0; k < R; k++) {
            const amp_t o = shfl_xor_amp(r[k], 1 << Q);
            r[k] = u_row(m0r, m0i, m1r, m1i, upper ? o : r[k], upper ? r[k] : o);
        }
    } else {
        constexpr int D = 1 << (Q - 6);
#pragma unroll
        for (int k = 0; k < R; k++)
            if ((k & D) == 0) u_butterfly(U, r[k], r[k + D]);
    }
}

template <int Q, int R, bool NT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_u_wave(amp_t *__restrict__ amp, UMat U, uint64_t ntiles, unsigned glog, unsigned slog)
{
    const unsigned lane = threadIdx.x & 63u;
    const uint64_t blk = stream_tile(glog, slog);
    const uint64_t wave = (blk * BLOCK + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * BLOCK) >> 6;
    for (uint64_t t = wave; t < ntiles; t += nwaves) {
        amp_t *base = amp + t * (64 * R) + lane;
        amp_t r[R];
#pragma unroll
        for (int k = 0; k < R; k++) r[k] = ld<NT>(base + k * 64);
        u_wave_tile<Q, R>(U, r, lane);
#pragma unroll
        for (int k = 0; k < R; k++) st<NT>(base + k * 64, r[k]);
    }
}

// K12c  controlled form with the control or the target below bit 3, i.e. inside a 128-B line (k_phase_lines' reason: one
// touched amplitude per lane would fetch 16 B out of every 32 or 64).  A lane owns one amplitude of every touched line:
//   LOWQ (q < 3, any c):  the partner sits in the same line and arrives by xor-shuffle, every lane computes its own row as in
//         K12b.  A control >= 3 is squeezed out of the numbering (count = 2^(n-1), only control-set lines are read, every lane
//         hits); a control < 3 leaves every line touched (count = 2^n) and the lanes with their control bit clear keep their value.
//   !LOWQ (c < 3 <= q):   a lane owns the pair (i0, i0 | 2^q), count = 2^(n-1); both lines are loaded whole, the lanes with bit c
//         set rotate.
// store_all: control at 16- or 32-B granularity -- whole lines are stored back, the untouched amplitudes with the bits they had
// (k_phase_lines measured masked 32-B stores at 4.0 ms against 2.6); a control at bit 2 stores its 64-B halves only.
// count is a multiple of 64 (the host asks for n >= 9), so a wave never diverges at the loop's end and the shuffle sees every lane.
template <bool LOWQ>
__global__ __launch_bounds__(64) void k_cu_lines(amp_t *__restrict__ amp, unsigned q, unsigned c, int store_all, UMat U,
                                                 uint64_t count, unsigned glog, unsigned slog)
{
    const uint64_t step = (uint64_t)gridDim.x * 64u;
    const uint64_t tile0 = stream_tile(glog, slog);
    for (uint64_t p = tile0 * 64u + threadIdx.x; p < count; p += step) {
        if (LOWQ) {
            uint64_t i = p;
            if (c >= 3) i = insert_zero(p, c) | ((uint64_t)1 << c);      // (bits below c keep their place: lane ^ 2^q holds the partner)
            const amp_t v = __builtin_nontemporal_load(amp + i);
            const amp_t o = shfl_xor_amp(v, 1 << q);
            const bool upper = (i >> q) & 1u, hit = (i >> c) & 1u;
            if (hit) {
                const amp_t w = u_row(upper ? U.r10 : U.r00, upper ? U.i10 : U.i00, upper ? U.r11 : U.r01, upper ? U.i11 : U.i01,
                                      upper ? o : v, upper ? v : o);
                __builtin_nontemporal_store(w, amp + i);
            } else if (store_all) __builtin_nontemporal_store(v, amp + i);
        } else {
            const uint64_t i0 = insert_zero(p, q), i1 = i0 | ((uint64_t)1 << q);
            amp_t a = __builtin_nontemporal_load(amp + i0), b = __builtin_nontemporal_load(amp + i1);
            const bool hit = (i0 >> c) & 1u;
            if (hit) u_butterfly(U, a, b);
            if (hit || store_all) { __builtin_nontemporal_store(a, amp + i0); __builtin_nontemporal_store(b, amp + i1); }
        }
    }
}

// ---------------------------------------------------------------------------
// K13  any two-qubit gate, plain or controlled (qcx_two_qubit_gate / qcx_c_two_qubit_gate, DESIGN s4.5g): the 4x4 matrix m on
// the quads (i, i | 2^lo, i | 2^hi, i | 2^lo | 2^hi), lo < hi, as the reference's mat-vec would apply it from sixteen stored
// triplets per quad taken in ascending state index (Q:396-413):
//     out_r = q_row(m[r][0] * x0, m[r][1] * x1, m[r][2] * x2, m[r][3] * x3),   products by q_mul (the pinned arithmetic),
// all sixteen entries multiplied out even where they are zero.  The host
// has already permuted the caller's matrix when qubit0 > qubit1 (P u P, P = the index swap 1 <-> 2): a kernel only sees
// lo < hi and matrix index k = bit(lo) + 2 * bit(hi).  The 32 components are kernel arguments (SGPRs), read with constant
// indices only -- a lane that needs "its own" row picks it with selects, never with a run-time index, so nothing goes to
// scratch.  No LDS, no table, one arithmetic path for every matrix.  A result is never -0 (as in K12), so K0c's invariant
// holds behind these kernels.
// ---------------------------------------------------------------------------
struct U4Mat { double m[32]; };                          // m[(4 * r + k) * 2 + (0: re, 1: im)]
struct U4Row { double r0, i0, r1, i1, r2, i2, r3, i3; };

template <int ROW> __device__ __forceinline__ U4Row u4_row_of(const U4Mat &U)
{
    return {U.m[8 * ROW], U.m[8 * ROW + 1], U.m[8 * ROW + 2], U.m[8 * ROW + 3], U.m[8 * ROW + 4], U.m[8 * ROW + 5], U.m[8 * ROW + 6], U.m[8 * ROW + 7]};
}

// the row of the lane's own amplitude: row = lb + 2 * hb (its bits lo and hi)
__device__ __forceinline__ U4Row u4_row_sel(const U4Mat &U, bool lb, bool hb)
{
#define QCX_U4_SEL(k) (hb ? (lb ? U.m[24 + k] : U.m[16 + k]) : (lb ? U.m[8 + k] : U.m[k]))
    return {QCX_U4_SEL(0), QCX_U4_SEL(1), QCX_U4_SEL(2), QCX_U4_SEL(3), QCX_U4_SEL(4), QCX_U4_SEL(5), QCX_U4_SEL(6), QCX_U4_SEL(7)};
#undef QCX_U4_SEL
}

// one row, the 4-column extension of u_row: x0 .. x3 = the quad's amplitudes in ascending index order
__device__ __forceinline__ amp_t u4_row(const U4Row &m, amp_t x0, amp_t x1, amp_t x2, amp_t x3)
{
    return q_row(q_mul(m.r0, m.i0, x0), q_mul(m.r1, m.i1, x1), q_mul(m.r2, m.i2, x2), q_mul(m.r3, m.i3, x3));
}

__device__ __forceinline__ void u4_quad(const U4Mat &U, amp_t &x0, amp_t &x1, amp_t &x2, amp_t &x3)
{
    const amp_t o0 = u4_row(u4_row_of<0>(U), x0, x1, x2, x3), o1 = u4_row(u4_row_of<1>(U), x0, x1, x2, x3);
    const amp_t o2 = u4_row(u4_row_of<2>(U), x0, x1, x2, x3), o3 = u4_row(u4_row_of<3>(U), x0, x1, x2, x3);
    x0 = o0; x1 = o1; x2 = o2; x3 = o3;
}

// K13a  quad form, any pair of targets (K12a's shape).  A lane owns one quad: four 16-B loads before the first store.  s0 < s1
// (< s2) are the squeezed-out index bits in ascending order: lo and hi, and with CTL the control, which is then set -- only
// the 2^(n-3) control-set quads are read or written.  count = 2^(n-2) (CTL: 2^(n-3)); stream-interleaved tile order as in
// k_phase; a partial last tile (count < BLOCK) is guarded by p < count.
template <bool NT, bool CTL, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_u2_quad(amp_t *__restrict__ amp, unsigned lo, unsigned hi, unsigned c, unsigned s0, unsigned s1,
                                                     unsigned s2, U4Mat U, uint64_t count, unsigned glog, unsigned slog)
{
    const uint64_t lob = (uint64_t)1 << lo, hib = (uint64_t)1 << hi;
    const uint64_t step = (uint64_t)gridDim.x * BLOCK;
    const uint64_t tile0 = stream_tile(glog, slog);
    for (uint64_t base = tile0 * BLOCK; base < count; base += step) {
        const uint64_t p = base + threadIdx.x;
        if (p < count) {
            uint64_t i = insert_zero(insert_zero(p, s0), s1);
            if (CTL) i = insert_zero(i, s2) | ((uint64_t)1 << c);
            amp_t x0 = ld<NT>(amp + i), x1 = ld<NT>(amp + (i | lob)), x2 = ld<NT>(amp + (i | hib)), x3 = ld<NT>(amp + (i | lob | hib));
            u4_quad(U, x0, x1, x2, x3);
            st<NT>(amp + i, x0); st<NT>(amp + (i | lob), x1); st<NT>(amp + (i | hib), x2); st<NT>(amp + (i | lob | hib), x3);
        }
    }
}

// K13b  line forms: lo, or the control, below bit 3, i.e. inside a 128-B line (K12b / K12c's reason: a wave memory instruction
// must cover whole lines).  A lane owns ONE amplitude of every touched line, and the four amplitudes of its quad reach it
//   - by xor-shuffle where the target sits below bit 6 of the lane numbering (NS of the two targets: lo first, lo < hi),
//   - as further registers of the same lane, loaded from the lines 2^hi (and 2^lo) away, where it sits above.
// Squeezed out of the numbering p (in ascending order s0 < s1, nsq of them): a control >= 3, which is then set (cset: only
// control-set lines are read), and the targets that live in registers.  Squeezing a control in 3 .. 5 moves the targets above
// it down by one lane bit: mlo / mhi are the shuffle masks in LANE numbering, the lane's own row comes from the bits of its
// INDEX.  Every lane computes its OWN row (NS = 2), its own two rows (NS = 1) or all four (NS = 0), the row's eight components
// chosen by its bits lo and hi, the four amplitudes fed in ascending index order -- so the sums are those of the definition.
// A control < 3 (clow = its bit, else 0) leaves every line touched: lanes whose control bit is clear keep their bits and, with
// store_all (control at 16- or 32-B granularity, as in k_cu_lines), whole lines are stored back.
// count is a multiple of 64 (the host asks for n >= 9 and squeezes at most two bits), so no wave diverges around a shuffle.
template <int NS, bool NT>
__global__ __launch_bounds__(64) void k_u2_lines(amp_t *__restrict__ amp, unsigned lo, unsigned hi, unsigned mlo, unsigned mhi, unsigned nsq,
                                                 unsigned s0, unsigned s1, uint64_t cset, unsigned clow, int store_all, U4Mat U,
                                                 uint64_t count, unsigned glog, unsigned slog)
{
    const uint64_t lob = (uint64_t)1 << lo, hib = (uint64_t)1 << hi;
    const uint64_t step = (uint64_t)gridDim.x * 64u;
    const uint64_t tile0 = stream_tile(glog, slog);
    for (uint64_t p = tile0 * 64u + threadIdx.x; p < count; p += step) {
        uint64_t i = p;
        if constexpr (NS == 0) i = insert_zero(insert_zero(p, lo), hi);      // (only with a control < 3: nothing else is squeezed out)
        else {
            if (nsq > 0) i = insert_zero(i, s0);
            if (nsq > 1) i = insert_zero(i, s1);
            i |= cset;
        }
        const bool hit = clow == 0 || (i & clow) != 0;
        const bool lb = (i & lob) != 0, hb = (i & hib) != 0;
        if constexpr (NS == 2) {
            const amp_t v = ld<NT>(amp + i);
            const amp_t ol = shfl_xor_amp(v, (int)mlo), oh = shfl_xor_amp(v, (int)mhi), olh = shfl_xor_amp(ol, (int)mhi);
            // a_j: bit lo = j & 1, bit hi = (own) ^ (j >> 1); then ascending order
            const amp_t a0 = lb ? ol : v, a1 = lb ? v : ol, a2 = lb ? olh : oh, a3 = lb ? oh : olh;
            if (hit) st<NT>(amp + i, u4_row(u4_row_sel(U, lb, hb), hb ? a2 : a0, hb ? a3 : a1, hb ? a0 : a2, hb ? a1 : a3));
            else if (store_all) st<NT>(amp + i, v);
        } else if constexpr (NS == 1) {                        // (i has bit hi clear: squeezed out)
            const amp_t v0 = ld<NT>(amp + i), v1 = ld<NT>(amp + (i | hib));
            const amp_t o0 = shfl_xor_amp(v0, (int)mlo), o1 = shfl_xor_amp(v1, (int)mlo);
            const amp_t x0 = lb ? o0 : v0, x1 = lb ? v0 : o0, x2 = lb ? o1 : v1, x3 = lb ? v1 : o1;
            if (hit) {
                st<NT>(amp + i, u4_row(u4_row_sel(U, lb, false), x0, x1, x2, x3));
                st<NT>(amp + (i | hib), u4_row(u4_row_sel(U, lb, true), x0, x1, x2, x3));
            } else if (store_all) { st<NT>(amp + i, v0); st<NT>(amp + (i | hib), v1); }
        } else {                                               // (bits lo and hi clear: both squeezed out)
            amp_t x0 = ld<NT>(amp + i), x1 = ld<NT>(amp + (i | lob)), x2 = ld<NT>(amp + (i | hib)), x3 = ld<NT>(amp + (i | lob | hib));
            if (hit) u4_quad(U, x0, x1, x2, x3);
            if (hit || store_all) { st<NT>(amp + i, x0); st<NT>(amp + (i | lob), x1); st<NT>(amp + (i | hib), x2); st<NT>(amp + (i | lob | hib), x3); }
        }
    }
}

// ---------------------------------------------------------------------------
// K17  a one- or two-qubit gate under any set of controls of either polarity (qcx_mc_one_qubit_gate / qcx_mc_two_qubit_gate,
// DESIGN s4.5m): K12's and K13's rows on the pairs / quads whose index satisfies (i & ctrl_mask) == ctrl_values, nothing else
// read.  The forms are K12a / K12c / K13a / K13b's with two generalisations, both decided on the host (qcx_mc_gate_plan):
//   the numbering.  Every control at bit >= 3 and every target that lives in registers is squeezed out of the work numbering:
//       index(p) = deposit(p) | orc,
//       deposit = p's bits moved, in order, into the positions that are NOT squeezed; the squeezed positions come as ascending
//       runs (position, length) in McMap, a by-value kernel argument -- no table in memory, nothing allocated; orc = the bits
//       of the positive squeezed controls.  A deposit is bit-wise: deposit(base + lane) = deposit(base) | deposit(lane) for a
//       tile base that is a multiple of 64, so the lane's part is formed once per kernel and the tile's part is wave-uniform
//       (scalar) work; the loop over the runs has the same trip count in every lane.
//   the predicate.  Controls below bit 3 leave every line touched: a lane hits when (i & lmask) == lvals (K12c / K13b's clow
//       test with a mask and values); bits 0-2 of an index are the lane's, so the test is formed once per kernel too.  Lanes
//       that miss keep their bits and, with store_all (a control at 16- or 32-B granularity), whole lines are stored back.
// A workgroup is one wave, a tile 64 work items; stream-interleaved tile order as in k_phase.  The shuffle forms are launched
// with a work count that is a multiple of 64 only (the host's rule), so no wave diverges around a shuffle.
// ---------------------------------------------------------------------------
constexpr unsigned MC_MAP_RUNS = 17;                       // QCX_MC_MAX_RUNS of include/qcx_plan.h (the host asserts that they agree)
struct McMap { uint32_t run[MC_MAP_RUNS]; uint32_t nruns; uint64_t orc; };      // run = position | length << 8, ascending

__device__ __forceinline__ uint64_t mc_deposit(const McMap &M, uint64_t p)
{
    uint64_t i = p;
    for (unsigned k = 0; k < M.nruns; k++) {
        const unsigned pos = M.run[k] & 255u, len = M.run[k] >> 8;
        const uint64_t low = ((uint64_t)1 << pos) - 1;
        i = ((i & ~low) << len) | (i & low);
    }
    return i;
}

// K17a  one target, the pair in two registers of a lane (K12a's shape; with lmask != 0 K12c's !LOWQ case).  The target is
// squeezed out: count pairs.  Correct for any bit positions (the small-count fallback squeezes every control, lmask = 0).
template <bool NT>
__global__ __launch_bounds__(64) void k_mcu_pair(amp_t *__restrict__ amp, unsigned q, McMap M, unsigned lmask, unsigned lvals, int store_all,
                                                 UMat U, uint64_t count, unsigned glog, unsigned slog)
{
    const uint64_t bit = (uint64_t)1 << q, step = (uint64_t)gridDim.x * 64u;
    const uint64_t lane_i = mc_deposit(M, threadIdx.x) | M.orc;
    const bool hit = ((unsigned)lane_i & lmask) == lvals;
    for (uint64_t base = stream_tile(glog, slog) * 64u; base < count; base += step) {
        if (base + threadIdx.x < count) {
            const uint64_t i0 = mc_deposit(M, base) | lane_i;
            amp_t a = ld<NT>(amp + i0), b = ld<NT>(amp + i0 + bit);
            if (hit) u_butterfly(U, a, b);
            if (hit || store_all) { st<NT>(amp + i0, a); st<NT>(amp + i0 + bit, b); }
        }
    }
}

// K17b  one target below bit 3: a lane owns one amplitude of every touched line, the partner arrives by xor-shuffle and every
// lane computes its own row (K12c's LOWQ case).  count is a multiple of 64.
template <bool NT>
__global__ __launch_bounds__(64) void k_mcu_shfl(amp_t *__restrict__ amp, unsigned q, McMap M, unsigned lmask, unsigned lvals, int store_all,
                                                 UMat U, uint64_t count, unsigned glog, unsigned slog)
{
    const uint64_t step = (uint64_t)gridDim.x * 64u;
    const uint64_t lane_i = mc_deposit(M, threadIdx.x) | M.orc;      // (bits below 3 keep their place: lane ^ 2^q holds the partner)
    const bool hit = ((unsigned)lane_i & lmask) == lvals, upper = (lane_i >> q) & 1u;
    const double m0r = upper ? U.r10 : U.r00, m0i = upper ? U.i10 : U.i00, m1r = upper ? U.r11 : U.r01, m1i = upper ? U.i11 : U.i01;
    for (uint64_t base = stream_tile(glog, slog) * 64u; base < count; base += step) {
        const uint64_t i = mc_deposit(M, base) | lane_i;
        const amp_t v = ld<NT>(amp + i);
        const amp_t o = shfl_xor_amp(v, 1 << q);
        if (hit) st<NT>(amp + i, u_row(m0r, m0i, m1r, m1i, upper ? o : v, upper ? v : o));
        else if (store_all) st<NT>(amp + i, v);
    }
}

// K17c  two targets, the quad in four registers of a lane (K13a's shape; with lmask != 0 K13b's NS = 0).  Both targets are
// squeezed out: count quads.  Correct for any bit positions (the small-count fallback squeezes every control, lmask = 0).
template <bool NT>
__global__ __launch_bounds__(64) void k_mcu2_quad(amp_t *__restrict__ amp, unsigned lo, unsigned hi, McMap M, unsigned lmask, unsigned lvals,
                                                  int store_all, U4Mat U, uint64_t count, unsigned glog, unsigned slog)
{
    const uint64_t lob = (uint64_t)1 << lo, hib = (uint64_t)1 << hi, step = (uint64_t)gridDim.x * 64u;
    const uint64_t lane_i = mc_deposit(M, threadIdx.x) | M.orc;
    const bool hit = ((unsigned)lane_i & lmask) == lvals;
    for (uint64_t base = stream_tile(glog, slog) * 64u; base < count; base += step) {
        if (base + threadIdx.x < count) {
            const uint64_t i = mc_deposit(M, base) | lane_i;
            amp_t x0 = ld<NT>(amp + i), x1 = ld<NT>(amp + (i | lob)), x2 = ld<NT>(amp + (i | hib)), x3 = ld<NT>(amp + (i | lob | hib));
            if (hit) u4_quad(U, x0, x1, x2, x3);
            if (hit || store_all) { st<NT>(amp + i, x0); st<NT>(amp + (i | lob), x1); st<NT>(amp + (i | hib), x2); st<NT>(amp + (i | lob | hib), x3); }
        }
    }
}

// K17d  two targets, line forms (K13b's NS = 2 and NS = 1): NS targets sit below bit 6 of the LANE numbering and reach the lane
// by xor-shuffle (mlo, mhi: the shuffle masks in lane numbering -- squeezing controls in 3 .. 5 moves the targets above them
// down); the other target, if any, is squeezed out and lives in a second register.  The lane's own row comes from the bits of
// its INDEX, the four amplitudes are fed in ascending index order.  count is a multiple of 64.
template <int NS, bool NT>
__global__ __launch_bounds__(64) void k_mcu2_lines(amp_t *__restrict__ amp, unsigned lo, unsigned hi, unsigned mlo, unsigned mhi, McMap M,
                                                   unsigned lmask, unsigned lvals, int store_all, U4Mat U, uint64_t count, unsigned glog, unsigned slog)
{
    const uint64_t lob = (uint64_t)1 << lo, hib = (uint64_t)1 << hi, step = (uint64_t)gridDim.x * 64u;
    const uint64_t lane_i = mc_deposit(M, threadIdx.x) | M.orc;      // (a target that is shuffled is a lane bit: its index bit is the lane's)
    const bool hit = ((unsigned)lane_i & lmask) == lvals, lb = (lane_i & lob) != 0, hb = NS == 2 && (lane_i & hib) != 0;
    for (uint64_t base = stream_tile(glog, slog) * 64u; base < count; base += step) {
        const uint64_t i = mc_deposit(M, base) | lane_i;
        if constexpr (NS == 2) {
            const amp_t v = ld<NT>(amp + i);
            const amp_t ol = shfl_xor_amp(v, (int)mlo), oh = shfl_xor_amp(v, (int)mhi), olh = shfl_xor_amp(ol, (int)mhi);
            // a_j: bit lo = j & 1, bit hi = (own) ^ (j >> 1); then ascending order
            const amp_t a0 = lb ? ol : v, a1 = lb ? v : ol, a2 = lb ? olh : oh, a3 = lb ? oh : olh;
            if (hit) st<NT>(amp + i, u4_row(u4_row_sel(U, lb, hb), hb ? a2 : a0, hb ? a3 : a1, hb ? a0 : a2, hb ? a1 : a3));
            else if (store_all) st<NT>(amp + i, v);
        } else {                                               // (i has bit hi clear: squeezed out)
            const amp_t v0 = ld<NT>(amp + i), v1 = ld<NT>(amp + (i | hib));
            const amp_t o0 = shfl_xor_amp(v0, (int)mlo), o1 = shfl_xor_amp(v1, (int)mlo);
            const amp_t x0 = lb ? o0 : v0, x1 = lb ? v0 : o0, x2 = lb ? o1 : v1, x3 = lb ? v1 : o1;
            if (hit) {
                st<NT>(amp + i, u4_row(u4_row_sel(U, lb, false), x0, x1, x2, x3));
                st<NT>(amp + (i | hib), u4_row(u4_row_sel(U, lb, true), x0, x1, x2, x3));
            } else if (store_all) { st<NT>(amp + i, v0); st<NT>(amp + (i | hib), v1); }
        }
    }
}

// K12s / K13s / K17s  a controlled gate as a STRICT pass (K9's reason: a register that holds non-finite amplitudes), for one
// control as for any mask: one plain pass over all pairs / quads, the defined rows where (i & cmask) == cvals, and every other
// amplitude rewritten through the reference's identity row q_row((1, 0) * x); `one` and `z` are kernel arguments so that no
// product is folded.  (The plain gates need no strict twin: every form of K12 and K13 multiplies every stored triplet out and
// rewrites every amplitude; the non-finite tests prove it.)
__global__ __launch_bounds__(256) void k_strict_mcu(amp_t *__restrict__ amp, unsigned n, unsigned q, uint64_t cmask, uint64_t cvals, UMat U,
                                                    double one, double z)
{
    const uint64_t half = (uint64_t)1 << (n - 1);
    for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < half; p += (uint64_t)gridDim.x * 256u) {
        const uint64_t i0 = insert_zero(p, q), i1 = i0 | ((uint64_t)1 << q);
        amp_t a = amp[i0], b = amp[i1];
        if ((i0 & cmask) == cvals) u_butterfly(U, a, b);
        else { a = q_row(q_mul(one, z, a)); b = q_row(q_mul(one, z, b)); }
        amp[i0] = a; amp[i1] = b;
    }
}

__global__ __launch_bounds__(256) void k_strict_mcu2(amp_t *__restrict__ amp, unsigned n, unsigned lo, unsigned hi, uint64_t cmask, uint64_t cvals,
                                                     U4Mat U, double one, double z)
{
    const uint64_t quads = (uint64_t)1 << (n - 2), lob = (uint64_t)1 << lo, hib = (uint64_t)1 << hi;
    for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < quads; p += (uint64_t)gridDim.x * 256u) {
        const uint64_t i = insert_zero(insert_zero(p, lo), hi);
        amp_t x[4] = {amp[i], amp[i | lob], amp[i | hib], amp[i | lob | hib]};
        if ((i & cmask) == cvals) u4_quad(U, x[0], x[1], x[2], x[3]);
        else {
#pragma unroll
            for (int k = 0; k < 4; k++) x[k] = q_row(q_mul(one, z, x[k]));
        }
        amp[i] = x[0]; amp[i | lob] = x[1]; amp[i | hib] = x[2]; amp[i | lob | hib] = x[3];
    }
}

// ---------------------------------------------------------------------------
// K15  the rotation about a Pauli string, exp(-i theta/2 P) = cos(theta/2) I - i sin(theta/2) P, in place (qcx_pauli_rotation,
// DESIGN s4.5i; tests/pauli_rotation_ref.py is the definition).  The string is K14's (x_mask, z_mask), g = popcount(x_mask &
// z_mask) mod 4, (c, s) = polar(theta / 2).  The matrix has one or two entries per row and is applied as the reference's
// mat-vec would apply it from stored triplets taken in ascending column order: rows by q_row, products by q_mul (the pinned
// arithmetic), zero components multiplied out:
//     (er, ei) = -i i^g s = (+0, -s), (s, +0), (+0, s), (-s, +0);   entry(i, j) = (er, ei), its ONE non-zero component negated
//     when popcount(j & z_mask) is odd (the other stays +0), j = i ^ x_mask
//     x_mask != 0:  D = (c, +0) * amp[i], O = entry(i, j) * amp[j],  new[i] = i < j ? q_row(D, O) : q_row(O, D)
//     x_mask == 0:  new[i] = q_row((c, -+s) * amp[i]), -s where popcount(i & z_mask) is even (this is entry(i, i) with re = c)
// What the definition is, bit for bit, on finite states (tests/test_pauli_rotation_ref.py, and on the GPU
// tests/test_gpu_pauli_rotation.py):
//     one letter on qubit q        = qcx_one_qubit_gate(q, .) with [[c, -is], [-is, c]] (X), [[c, -s], [s, c]] (Y),
//                                    diag(c - is, c + is) (Z)
//     two letters on qubits q0, q1 = qcx_two_qubit_gate(q0, q1, .) with c I - i s P built component by component, either order
//     and cos(theta/2) I - i sin(theta/2) P as a dense matrix to 1e-14 on O(1) amplitudes.
// Every amplitude is rewritten from its own row's products: a result is never -0 (K0c's invariant holds behind this kernel),
// and an Inf or NaN reaches rows i and i ^ x_mask only -- there is no strict twin.
// The units of work, the partner's addresses and the sign bitmaps are PauliTiles' (shared with K14):
//   SHAPE 0  a tile, x_mask == 0: a streaming diagonal, the sign from the index parity; no LDS
//   SHAPE 1  a tile, the partner inside it (x_mask < 2^T): the tile goes through LDS once (64 KiB), whole 128-B lines in and
//            out; behind the barrier -- the whole tile is in LDS before any of its stores is issued -- the next tile's loads
//            go out, a thread reads e and e ^ x_low back, computes its OWN row and stores its own element
//   SHAPE 2  the PAIR of tiles (t, t ^ xh): a at e of tile t, b at e ^ x_low of the partner.  i < j on t's side always: a takes D then O, b
//            takes O then D; both are stored where they came from.  Units are disjoint, so in place is safe; no LDS.
// SHAPE 0 and 2 hold no more than 8 elements of a thread at a time (8 a's and 8 b's: 64 VGPRs) and prefetch nothing: there is
// no barrier in them, so the other waves of the CU cover the latency (2, 4 and 16 elements at a time measured the same at
// n = 30, DESIGN s4.5i).  FULL as in K14: !FULL is the one partial tile of n < 12.
// ---------------------------------------------------------------------------
struct PRot { double c, zr, er, ei; };                   // zr = the +0 imaginary part of the diagonal (an argument: never folded)

// entry * x with the entry's sign applied to its non-zero component (er for odd g, ei for even g)
__device__ __forceinline__ q_mul prot_off(const PRot &R, bool godd, bool neg, amp_t x)
{
    return q_mul((godd && neg) ? -R.er : R.er, (!godd && neg) ? -R.ei : R.ei, x);
}

// the row of `own`: first = its index is below the partner's (the diagonal triplet comes first)
__device__ __forceinline__ amp_t prot_row(const PRot &R, bool godd, bool neg, bool first, amp_t own, amp_t oth)
{
    const q_mul d(R.c, R.zr, own), o = prot_off(R, godd, neg, oth);
    const amp_t d_first = q_row(d, o), o_first = q_row(o, d);      // (both, then a select: `first` differs from lane to lane)
    return first ? d_first : o_first;
}

// x_mask == 0: the one triplet (c, -+s) (g = 0: ei = -s carries the sign)
__device__ __forceinline__ amp_t prot_diag(const PRot &R, bool neg, amp_t x)
{
    return q_row(q_mul(R.c, neg ? -R.ei : R.ei, x));
}

template <int SHAPE, bool FULL>
__global__ __launch_bounds__(256) void k_pauli_rot(amp_t *__restrict__ amp, uint64_t nunits, unsigned T, uint64_t x_mask,
                                                   uint64_t z_mask, unsigned g, PRot R)
{
    using Tiles = PauliTiles<SHAPE == 2>;
    constexpr unsigned EPT = Tiles::EPT, HALF = 8u;
    const unsigned tid = threadIdx.x;
    const Tiles P(T, x_mask, z_mask, tid);
    const unsigned x_low = P.x_low, nld = P.nld, podd = P.podd, sodd = P.sodd;      // (SHAPE 2 needs both bitmaps)
    const bool godd = (g & 1u) != 0;
    if constexpr (SHAPE == 1) {
        __shared__ amp_t sa[4096];
        const unsigned hbit = 1u << (31u - (unsigned)__clz((int)x_low));      // (SHAPE 1: x_low != 0) i < j <=> this bit of e is clear
        amp_t a[EPT];
        auto load = [&](uint64_t u) {
            const amp_t *pa = amp + (u << T) + tid;
#pragma unroll
            for (unsigned j = 0; j < EPT; j++)
                if (FULL || j < nld) a[j] = __builtin_nontemporal_load(pa + 256u * j);
        };
        if (blockIdx.x < nunits) load(blockIdx.x);
        for (uint64_t u = blockIdx.x; u < nunits; u += gridDim.x) {
            const unsigned tile_par = P.par(u);                              // (xh == 0: the partner's tile is this one)
#pragma unroll
            for (unsigned j = 0; j < EPT; j++)
                if (FULL || j < nld) sa[tid + 256u * j] = a[j];
            __syncthreads();
            if (u + gridDim.x < nunits) load(u + gridDim.x);
            amp_t *po = amp + (u << T) + tid;
#pragma unroll
            for (unsigned j = 0; j < EPT; j++)
                if (FULL || j < nld) {
                    const unsigned e = tid + 256u * j;
                    const amp_t r = prot_row(R, godd, ((tile_par + (podd >> j)) & 1u) != 0, (e & hbit) == 0, sa[e], sa[e ^ x_low]);
                    __builtin_nontemporal_store(r, po + 256u * j);
                }
            __syncthreads();
        }
    } else if constexpr (SHAPE == 0) {
        for (uint64_t u = blockIdx.x; u < nunits; u += gridDim.x) {
            const unsigned tile_par = P.par(u);
            amp_t *pa = amp + (u << T) + tid;
#pragma unroll 1
            for (unsigned h = 0; h < EPT; h += HALF) {
                amp_t a[HALF];
#pragma unroll
                for (unsigned k = 0; k < HALF; k++)
                    if (FULL || h + k < nld) a[k] = __builtin_nontemporal_load(pa + 256u * (h + k));
#pragma unroll
                for (unsigned k = 0; k < HALF; k++)
                    if (FULL || h + k < nld)
                        __builtin_nontemporal_store(prot_diag(R, ((tile_par + (sodd >> (h + k))) & 1u) != 0, a[k]), pa + 256u * (h + k));
            }
        }
    } else {
        for (uint64_t u = blockIdx.x; u < nunits; u += gridDim.x) {                  // (SHAPE 2: xh != 0, n > 12, whole tiles)
            const uint64_t t = P.tile_of(u);
            const unsigned par_a = P.par(t), par_b = P.par(t ^ P.xh);
            amp_t *pa = amp + (t << T) + tid;
            amp_t *pb = amp + ((t ^ P.xh) << T) + P.partner_lane(tid);
#pragma unroll 1
            for (unsigned h = 0; h < EPT; h += HALF) {
                amp_t a[HALF], b[HALF];
#pragma unroll
                for (unsigned k = 0; k < HALF; k++) {
                    a[k] = __builtin_nontemporal_load(pa + 256u * (h + k));
                    b[k] = __builtin_nontemporal_load(pb + 256u * P.partner_elem(h + k));
                }
#pragma unroll
                for (unsigned k = 0; k < HALF; k++) {
                    // a's row meets b's index in the entry's sign, and the other way round
                    const amp_t ra = prot_row(R, godd, ((par_b + (podd >> (h + k))) & 1u) != 0, true, a[k], b[k]);
                    const amp_t rb = prot_row(R, godd, ((par_a + (sodd >> (h + k))) & 1u) != 0, false, b[k], a[k]);
                    __builtin_nontemporal_store(ra, pa + 256u * (h + k));
                    __builtin_nontemporal_store(rb, pb + 256u * P.partner_elem(h + k));
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// K15b  a RUN of K15's rotations in one read and one write of the state (qcx_pauli_rotation_batch, DESIGN s4.5k): up to
// QCX_PROT_RUN_W consecutive terms of a list whose partners i ^ x_mask all stay inside one tile of 2^12 amplitudes, applied in
// the order given while the tile sits in registers -- term by term K15's arithmetic (prot_diag / prot_row), so the state
// afterwards is, bit for bit, what one k_pauli_rot launch per term leaves.  Terms need not commute: only locality is used.
// The tile is NOT the 12 lowest index bits: it is bits 0-7 plus the pass's four HOT bits hot[0] < .. < hot[3], any in [8, n)
// (qcx_pauli_rotation_batch_plan chooses them from the strings).  Thread tid holds the tile-local elements e = tid + 256 j, j < 16,
// for all terms; element e of unit u is index base(u) + tid + off(j): off(j) deposits j's four bits at the hot bits (uniform),
// base(u) deposits u into the n - 12 bits that are left, so a wave instruction still moves one whole run of 2^8 amplitudes'
// quarter, 1 KiB.  Units are disjoint index sets: in place is safe.  The deposit is monotone, so tile-local order is index order.
// A term arrives as a record in the kernel arguments (uniform index: scalar loads, no table in memory), its masks already
// tile-local:
//     loc = x_loc | z_loc << 12 | g << 24   (x_loc, z_loc: bits 0-7 of the mask, and its hot bits at 8-11)
//     odd: bit j = par(j & (z_loc >> 8)), the thread's own element; bit 16 + j = par((e ^ x_loc) & z_loc) - par(tid & z_loc),
//          its partner's -- the entry's sign goes by the PARTNER's index, as K15's podd
//     popcount(i & z_mask) mod 2 = par(base(u) & z_mask) + par(tid & z_loc) + bit j of odd
//   x_loc == 0  prot_diag on the 16 registers: no LDS, no barrier
//   else        own elements to LDS (64 KiB), barrier, the partner read back from e ^ x_loc, prot_row with first = the highest
//               bit of x_loc is clear in e; a barrier before the next term's writes.  Where x_loc has hot bits only, the partner
//               is the thread's own element j ^ (x_loc >> 8) and nothing leaves the registers (the same prot_row: the same bits)
// DIAG: the pass has no exchange term, and the kernel no LDS at all.  FULL as in K15: !FULL is the one partial tile of n < 12
// (hot = 8 .. 11, elements at or above 2^n guarded).
// ---------------------------------------------------------------------------
#define QCX_PROT_RUN_W 32
struct PRotTerm {
    uint64_t z_mask;
    PRot     R;
    uint32_t loc, odd;
};
struct PRotRun { PRotTerm t[QCX_PROT_RUN_W]; };

// v with its sign bit flipped where bit 31 of sgn is set: "neg ? -v : v" for every v (a zero's and a NaN's sign included), as
// one 32-bit XOR, so that a sign put together from uniform and per-lane parts costs no compare and no select
__device__ __forceinline__ double prot_flip(double v, unsigned sgn)
{
    return __hiloint2double(__double2hiint(v) ^ (int)sgn, __double2loint(v));
}

template <bool DIAG, bool FULL>
__global__ __launch_bounds__(256) void k_prot_run(amp_t *__restrict__ amp, uint64_t nunits, unsigned n, unsigned hot, unsigned nterms,
                                                  PRotRun run)
{
    constexpr unsigned EPT = 16u;
    __shared__ amp_t sa[DIAG ? 1 : 4096];
    const unsigned tid = threadIdx.x;
    const unsigned h0 = hot & 255u, h1 = (hot >> 8) & 255u, h2 = (hot >> 16) & 255u, h3 = hot >> 24;
    const unsigned nel = FULL ? 4096u : 1u << n;
    auto off = [&](unsigned j) {
        return ((uint64_t)(j & 1u) << h0) | ((uint64_t)((j >> 1) & 1u) << h1) | ((uint64_t)((j >> 2) & 1u) << h2) | ((uint64_t)(j >> 3) << h3);
    };
    for (uint64_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const uint64_t base = insert_zero(insert_zero(insert_zero(insert_zero(u << 8, h0), h1), h2), h3);
        amp_t a[EPT];
#pragma unroll
        for (unsigned j = 0; j < EPT; j++)
            if (FULL || tid + 256u * j < nel) a[j] = __builtin_nontemporal_load(amp + (base | off(j)) + tid);      // (a uniform address + the lane)
            else a[j] = amp_t{0.0, 0.0};                             // (never stored; the in-thread exchange moves it about)
#pragma unroll 1
        for (unsigned k = 0; k < nterms; k++) {
            const PRot R = run.t[k].R;
            const unsigned loc = run.t[k].loc, odd = run.t[k].odd;
            const unsigned x_loc = loc & 0xFFFu, z_loc = (loc >> 12) & 0xFFFu;
            // signs as words with bit 31 alone: the unit's and the lane's share of the parity here, element j's from `odd` (uniform)
            const unsigned parw = ((unsigned)__popcll(base & run.t[k].z_mask) + (unsigned)__popc(tid & z_loc)) << 31;
            auto oddw = [&](unsigned bit) { return ((odd >> bit) & 1u) << 31; };
            if (DIAG || x_loc == 0) {
                const double ei = prot_flip(R.ei, parw);
#pragma unroll
                for (unsigned j = 0; j < EPT; j++)
                    if (FULL || tid + 256u * j < nel) a[j] = prot_diag({R.c, R.zr, R.er, prot_flip(ei, oddw(j))}, false, a[j]);
            } else {
                const bool godd = ((loc >> 24) & 1u) != 0;
                const unsigned mr = godd ? 0x80000000u : 0u, mi = mr ^ 0x80000000u;      // the entry's non-zero component carries the sign
                const double er = prot_flip(R.er, parw & mr), ei = prot_flip(R.ei, parw & mi);
                const unsigned hbit = 1u << (31u - (unsigned)__clz((int)x_loc));
                if ((x_loc & 255u) == 0) {
                    // the partner is one of the thread's own elements, j ^ (x_loc >> 8): b = a so permuted, one uniform step
                    // per hot bit of x_loc, and neither LDS nor a barrier
                    amp_t b[EPT];
#pragma unroll
                    for (unsigned j = 0; j < EPT; j++) b[j] = a[j];
#pragma unroll
                    for (unsigned t = 0; t < 4; t++)
                        if ((x_loc >> (8u + t)) & 1u) {
#pragma unroll
                            for (unsigned j = 0; j < EPT; j++)
                                if (!((j >> t) & 1u)) { const amp_t v = b[j]; b[j] = b[j | (1u << t)]; b[j | (1u << t)] = v; }
                        }
#pragma unroll
                    for (unsigned j = 0; j < EPT; j++)
                        if (FULL || tid + 256u * j < nel) {
                            const unsigned w = oddw(16u + j);
                            a[j] = prot_row({R.c, R.zr, prot_flip(er, w & mr), prot_flip(ei, w & mi)}, godd, false, ((256u * j) & hbit) == 0, a[j], b[j]);
                        }
                    continue;
                }
#pragma unroll
                for (unsigned j = 0; j < EPT; j++)
                    if (FULL || tid + 256u * j < nel) sa[tid + 256u * j] = a[j];
                __syncthreads();
#pragma unroll
                for (unsigned j = 0; j < EPT; j++)
                    if (FULL || tid + 256u * j < nel) {
                        const unsigned e = tid + 256u * j, w = oddw(16u + j);
                        a[j] = prot_row({R.c, R.zr, prot_flip(er, w & mr), prot_flip(ei, w & mi)}, godd, false, (e & hbit) == 0, a[j], sa[e ^ x_loc]);
                    }
                __syncthreads();
            }
        }
#pragma unroll
        for (unsigned j = 0; j < EPT; j++)
            if (FULL || tid + 256u * j < nel) __builtin_nontemporal_store(a[j], amp + (base | off(j)) + tid);
    }
}

// ---------------------------------------------------------------------------
// K12b / K13b  a RUN of K12's and K13's gates in one read and one write of the state (qcx_gate_batch, DESIGN s4.5l): consecutive
// gates of a list whose targets all lie inside one tile of 2^12 amplitudes, applied in the order given while the tile sits in
// registers.  Every output amplitude is its own row of the pinned arithmetic (u_row / u4_row: q_row over q_mul, columns in
// ascending index order), which lane computes a row changes no bit, so the state afterwards is what one launch per gate leaves.
// Tile, elements and addressing are k_prot_run's: bits 0-7 plus the pass's four hot bits, thread tid holds e = tid + 256 j,
// j < 16, index base(u) | off(j) | tid.
// The records travel in the kernel arguments in UNITS of 80 bytes and are read at a uniform running offset (scalar loads, no table
// in memory, nothing indexed at run time).  A record is a 16-byte header and the matrix: a one-target gate is 1 unit (UMat's 8
// doubles), a two-target gate 4 units (U4Mat's 32 doubles, already P u P where qubit0 > qubit1: 272 of the 320 bytes used).
//     header word 0:  p0 | p1 << 8 | cloc << 16 | cfull << 24 | ntargets << 32
//         p0 (< p1): the targets' tile-local positions (0-7 themselves, 8 + k = hot bit k)
//         cfull: the control as a bit of the full index, 255 = none; cloc: its tile-local position, 255 = not in the tile
//   control  an amplitude whose control bit is clear keeps the bits it has.  In the unit's base bits: the gate is skipped for
//            the whole unit; on a hot bit: skipped by j; in bits 0-7: a per-lane select (every lane still reaches the barriers)
//   all targets hot   the pair / quad is the thread's own registers: u_butterfly / u4_quad, no LDS, no barrier.  Two targets are
//            first brought to j's bits 0 and 1 by uniform register swaps (and back afterwards), so one copy of the quad code serves
//   one target in 0-5 the partner sits in the same wave: an xor-shuffle (k_u_wave's way), no LDS write and no barrier; the row as below
//   a target in 0-7   (any other) own elements to LDS (64 KiB), barrier, the pair's / quad's members read back in ascending order, the row of
//            the thread's own element chosen with selects (one target: (u00, u01) or (u10, u11) by its target bit; two: row
//            lb + 2 hb), a barrier before the next gate's writes
// LDS = false: every gate of the pass has hot targets only, and the kernel no LDS at all.  FULL as in K15b.
// ---------------------------------------------------------------------------
#define QCX_GATE_RUN_W 40                                  /* units in one pass: 3200 of the 4096 bytes of kernel arguments */
#define QCX_GATE_UNIT 10                                   /* 64-bit words in a unit */
struct GateRun { uint64_t w[QCX_GATE_RUN_W * QCX_GATE_UNIT]; };

// a[j] <-> a[j with bits BL and BH exchanged], for the j whose two bits differ: a uniform permutation of the thread's registers
#define QCX_GATE_SWAP(BL, BH)                                                                                   \
    _Pragma("unroll") for (unsigned j = 0; j < EPT; j++)                                                        \
        if (((j >> (BL)) & 1u) && !((j >> (BH)) & 1u)) {                                                        \
            const amp_t v = a[j]; a[j] = a[j ^ (1u << (BL)) ^ (1u << (BH))]; a[j ^ (1u << (BL)) ^ (1u << (BH))] = v; \
        }

template <bool LDS, bool FULL>
__global__ __launch_bounds__(256) void k_gate_run(amp_t *__restrict__ amp, uint64_t nunits, unsigned n, unsigned hot, unsigned ngates,
                                                  GateRun run)
{
    constexpr unsigned EPT = 16u;
    __shared__ amp_t sa[LDS ? 4096 : 1];
    const unsigned tid = threadIdx.x;
    const unsigned h0 = hot & 255u, h1 = (hot >> 8) & 255u, h2 = (hot >> 16) & 255u, h3 = hot >> 24;
    const unsigned nel = FULL ? 4096u : 1u << n;
    auto off = [&](unsigned j) {
        return ((uint64_t)(j & 1u) << h0) | ((uint64_t)((j >> 1) & 1u) << h1) | ((uint64_t)((j >> 2) & 1u) << h2) | ((uint64_t)(j >> 3) << h3);
    };
    auto mat = [&](unsigned at) { return __longlong_as_double((long long)run.w[at]); };
    auto pick = [](bool c, amp_t x, amp_t y) { return c ? x : y; };
    for (uint64_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const uint64_t base = insert_zero(insert_zero(insert_zero(insert_zero(u << 8, h0), h1), h2), h3);
        amp_t a[EPT];
#pragma unroll
        for (unsigned j = 0; j < EPT; j++)
            if (FULL || tid + 256u * j < nel) a[j] = __builtin_nontemporal_load(amp + (base | off(j)) + tid);
            else a[j] = amp_t{0.0, 0.0};                             // (never stored)
        unsigned at = 0;
#pragma unroll 1
        for (unsigned k = 0; k < ngates; k++) {
            const uint64_t hdr = run.w[at];
            const unsigned g = at + 2u, nt = (unsigned)(hdr >> 32);
            at += nt == 2u ? 4u * QCX_GATE_UNIT : QCX_GATE_UNIT;
            const unsigned p0 = (unsigned)hdr & 255u, p1 = (unsigned)(hdr >> 8) & 255u, cloc = (unsigned)(hdr >> 16) & 255u, cfull = (unsigned)(hdr >> 24) & 255u;
            if (cfull != 255u && cloc == 255u && !((base >> cfull) & 1u)) continue;      // a control in the base bits, clear: not this unit
            const unsigned cl = cloc < 8u ? 1u << cloc : 0u;                              // the control among the lane's bits ...
            unsigned ch = (cloc >= 8u && cloc < 12u) ? 1u << (cloc - 8u) : 0u;            // ... or among j's
            const bool lane_ok = (tid & cl) == cl;
            if (nt != 2u) {
                const UMat U = {mat(g), mat(g + 1), mat(g + 2), mat(g + 3), mat(g + 4), mat(g + 5), mat(g + 6), mat(g + 7)};
                if (!LDS || p0 >= 8u) {
#pragma unroll
                    for (unsigned t = 0; t < 4; t++)
                        if (p0 == 8u + t) {
#pragma unroll
                            for (unsigned j = 0; j < EPT; j++)
                                if (!((j >> t) & 1u) && (j & ch) == ch) {
                                    amp_t x = a[j], y = a[j | (1u << t)];
                                    u_butterfly(U, x, y);
                                    a[j] = pick(lane_ok, x, a[j]); a[j | (1u << t)] = pick(lane_ok, y, a[j | (1u << t)]);
                                }
                        }
                } else if constexpr (LDS) {
                    const bool upper = (tid >> p0) & 1u;
                    const double m0r = upper ? U.r10 : U.r00, m0i = upper ? U.i10 : U.i00;
                    const double m1r = upper ? U.r11 : U.r01, m1i = upper ? U.i11 : U.i01;
                    const unsigned bit = 1u << p0;
                    if (p0 < 6u) {
                        // the partner sits in the same wave: an xor-shuffle, neither an LDS write nor a barrier (k_u_wave's way).  Every
                        // lane shuffles, also one past a partial tile: its value is never used
#pragma unroll
                        for (unsigned j = 0; j < EPT; j++)
                            if ((j & ch) == ch) {
                                const amp_t o = shfl_xor_amp(a[j], (int)bit);
                                a[j] = pick(lane_ok, u_row(m0r, m0i, m1r, m1i, pick(upper, o, a[j]), pick(upper, a[j], o)), a[j]);
                            }
                        continue;
                    }
#pragma unroll
                    for (unsigned j = 0; j < EPT; j++)
                        if (FULL || tid + 256u * j < nel) sa[tid + 256u * j] = a[j];
                    __syncthreads();
#pragma unroll
                    for (unsigned j = 0; j < EPT; j++)
                        if ((FULL || tid + 256u * j < nel) && (j & ch) == ch) {
                            const amp_t o = sa[(tid + 256u * j) ^ bit];
                            a[j] = pick(lane_ok, u_row(m0r, m0i, m1r, m1i, pick(upper, o, a[j]), pick(upper, a[j], o)), a[j]);
                        }
                    __syncthreads();
                }
            } else {
                U4Mat U;
#pragma unroll
                for (unsigned c = 0; c < 32; c++) U.m[c] = mat(g + c);
                if (!LDS || p0 >= 8u) {
                    const unsigned t0 = p0 - 8u, t1 = p1 - 8u;       // t0 < t1: to j's bits 0 and 1
                    auto swapbits = [](unsigned v, unsigned x, unsigned y) { const unsigned d = ((v >> x) ^ (v >> y)) & 1u; return v ^ (d << x) ^ (d << y); };
                    ch = swapbits(swapbits(ch, 0u, t0 & 3u), 1u, t1 & 3u);
                    if (t0 == 1u) { QCX_GATE_SWAP(0, 1) }
                    if (t0 == 2u) { QCX_GATE_SWAP(0, 2) }
                    if (t1 == 2u) { QCX_GATE_SWAP(1, 2) }
                    if (t1 == 3u) { QCX_GATE_SWAP(1, 3) }
                    if (t0 < t1 && t1 < 4u) {
#pragma unroll
                        for (unsigned j = 0; j < EPT; j += 4)
                            if ((j & ch) == ch) {
                                amp_t x0 = a[j], x1 = a[j + 1], x2 = a[j + 2], x3 = a[j + 3];
                                u4_quad(U, x0, x1, x2, x3);
                                a[j] = pick(lane_ok, x0, a[j]); a[j + 1] = pick(lane_ok, x1, a[j + 1]);
                                a[j + 2] = pick(lane_ok, x2, a[j + 2]); a[j + 3] = pick(lane_ok, x3, a[j + 3]);
                            }
                    }
                    if (t1 == 3u) { QCX_GATE_SWAP(1, 3) }
                    if (t1 == 2u) { QCX_GATE_SWAP(1, 2) }
                    if (t0 == 2u) { QCX_GATE_SWAP(0, 2) }
                    if (t0 == 1u) { QCX_GATE_SWAP(0, 1) }
                } else if constexpr (LDS) {
                    const bool lb = (tid >> p0) & 1u;
                    const U4Row R0 = u4_row_sel(U, lb, false), R1 = u4_row_sel(U, lb, true);      // the rows of hb = 0 and of hb = 1
                    auto row = [&](bool hb) {
                        return U4Row{hb ? R1.r0 : R0.r0, hb ? R1.i0 : R0.i0, hb ? R1.r1 : R0.r1, hb ? R1.i1 : R0.i1,
                                     hb ? R1.r2 : R0.r2, hb ? R1.i2 : R0.i2, hb ? R1.r3 : R0.r3, hb ? R1.i3 : R0.i3};
                    };
                    const unsigned lob = 1u << p0, hib = 1u << p1;
#pragma unroll
                    for (unsigned j = 0; j < EPT; j++)
                        if (FULL || tid + 256u * j < nel) sa[tid + 256u * j] = a[j];
                    __syncthreads();
                    auto quad = [&](const U4Row &R, unsigned j) {
                        const unsigned e0 = (tid + 256u * j) & ~(lob | hib);
                        a[j] = pick(lane_ok, u4_row(R, sa[e0], sa[e0 | lob], sa[e0 | hib], sa[e0 | lob | hib]), a[j]);
                    };
                    if (p1 < 8u) {                                   // hb is the lane's
                        const U4Row R = row((tid >> p1) & 1u);
#pragma unroll
                        for (unsigned j = 0; j < EPT; j++)
                            if ((FULL || tid + 256u * j < nel) && (j & ch) == ch) quad(R, j);
                    } else {                                         // hb is j's: uniform
#pragma unroll
                        for (unsigned j = 0; j < EPT; j++)
                            if ((FULL || tid + 256u * j < nel) && (j & ch) == ch) quad(row((j >> (p1 - 8u)) & 1u), j);
                    }
                    __syncthreads();
                }
            }
        }
#pragma unroll
        for (unsigned j = 0; j < EPT; j++)
            if (FULL || tid + 256u * j < nel) __builtin_nontemporal_store(a[j], amp + (base | off(j)) + tid);
    }
}
#undef QCX_GATE_SWAP

// ---------------------------------------------------------------------------
// K16  the first stage of a qubit range's reduced density matrix (qcx_reduced_density_matrix, DESIGN s4.5j; tests/rdm_ref.py is
// the definition).  The range is [first, first + NUM), NV = 2^NUM its values; with a = amp[r, v], b = amp[r, w] (r = the bits
// outside the range, squeezed) the components are ROWS of an NV x NV table of doubles:
//     row v * NV + w, v <= w:  the real part, leaf  a.re b.re + a.im b.im           (v == w: the marginal's |a|^2)
//     row w * NV + v, v <  w:  the imaginary part of rho[v][w], leaf  a.im b.re - a.re b.im
// every product and sum rounded on its own (no FMA), and each row is K10's pairwise tree over r, lowest summed bit first.  A
// leaf's "0.0 +" waits until the unit's root, as in K14b: with signed-zero leaves a node differs from the canonical tree only
// where it is a zero of the other sign, and 0.0 + root is the same +0.
// A UNIT of work is 2^12 amplitudes: the range's NUM bits and the S = 12 - NUM lowest summed bits.  Those are the index bits
// [0, 12) when the range begins below S (EXCH), else the bits [0, S) and the range, unit u filling the bits between and above
// (whole runs of 2^S >= 256 amplitudes either way: a wave instruction reads 1 KiB).  A workgroup takes 2^ug CONSECUTIVE units, a
// GROUP -- ug more summed bits, the lowest that are left --, and thread k < NR adds their roots of row k as the tree does: a
// binary counter of partial sums (stack[l] = the sum of a finished block of 2^l units, joined with the next block of its size as
// soon as that is complete; unit i closes the blocks of its trailing one bits), so only a group's root leaves the kernel.
// Group g's root of row k goes to dst[k * row_stride + g], g = the summed bits left, in ascending order; the later stages are
// k_marginal<MARG_DBL> launches over all rows at once (the row number = kept high bits).
// Thread tid holds, after the loads (EXCH: after the unit's amplitudes changed hands through LDS once, padded as K14b's),
// x[v * C + c] = amp[r = tid + 256 c, v] for every v and the C = 16 / NV values of c: r's bits 0-5 are the lane, 6-7 the wave,
// 8.. are c.  It forms its NR * C = 2^(NUM + 4) leaves in groups of at most 64 and reduces a group over the lanes -- r's bits
// 0 - 5, in that order -- by HALVING: at level l a lane keeps the half of its values that bit l of its number selects, hands the
// other half to lane ^ 2^l and adds what it receives (IEEE addition commutes), so after the group's levels a lane holds one
// value, the wave's sum of the group's component number bit-reverse(lane).  That is 63 exchanges for 64 components where a
// butterfly per component would take 384, and no per-thread running sum.  Then one double per wave, component and c through LDS
// (ws), ONE barrier per unit, and thread k < NR forms row k: (w0 + w1) + (w2 + w3) per c -- r's bits 6, 7 --, then the tree over
// c -- r's bits 8 and up.  FULL tiles only (n >= 12): nothing in a unit's path is guarded, and the next unit's loads go out
// before the leaves are formed.  Nothing is written but dst.
// k_rdm_small is the one partial unit of a register below 12 qubits: the state in LDS, the leaves of as many rows as fit 2^12
// doubles at a time, K14's tree levels on them.
// ---------------------------------------------------------------------------
#define QCX_RDM_MAX_QUBITS 4
#define QCX_RDM_MAX_GROUP_BITS 4

__device__ __forceinline__ double rdm_xor_lane(double v, unsigned lvl)
{
    if (lvl == 0) return pauli_dpp<PAULI_DPP_XOR1>(v);
    if (lvl == 1) return pauli_dpp<PAULI_DPP_XOR2>(v);
    return __shfl_xor(v, 1 << lvl);
}

template <int NUM, bool EXCH>
__global__ __launch_bounds__(256) void k_rdm_leaves(const amp_t *__restrict__ amp, double *__restrict__ dst, uint64_t row_stride,
                                                    uint64_t ngroups, unsigned ug, unsigned first)
{
    static_assert(NUM >= 0 && NUM <= QCX_RDM_MAX_QUBITS, "a thread's 16 elements hold every value of the range");
    constexpr unsigned EPT = 16u, NV = 1u << NUM, NR = NV * NV, S = 12u - NUM, C = EPT / NV;
    constexpr unsigned NVAL = NR * C, GROUP = NVAL < 64u ? NVAL : 64u, NG = NVAL / GROUP;
    constexpr unsigned HL = GROUP == 64u ? 6u : (GROUP == 32u ? 5u : 4u);      // halving levels of a group
    static_assert((1u << HL) == GROUP, "a group is 16, 32 or 64 values");
    __shared__ __attribute__((aligned(16))) amp_t sa[EXCH ? 256u * 17u : 1u];
    __shared__ double ws[4u * NVAL];                                 // [wave][c * NR + row]
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t lowm = EXCH ? 0u : (((uint64_t)1) << (first - S)) - 1u;
    auto amp_pos = [](unsigned e) { return e + (e >> 4); };
    // the component a lane holds after a group's levels: bit l of the lane picked bit HL - 1 - l of the index
    unsigned held = 0;
#pragma unroll
    for (unsigned l = 0; l < HL; l++) held |= ((lane >> l) & 1u) << (HL - 1u - l);
    amp_t a[EPT];
    auto load = [&](uint64_t u) {
        const uint64_t base = EXCH ? u << 12 : (((u & lowm) << S) | ((u >> (first - S)) << (first + NUM)));
        const amp_t *p = amp + base + tid;
#pragma unroll
        for (unsigned j = 0; j < EPT; j++) {
            // element tid + 256 j of the unit, in memory order
            const uint64_t o = EXCH ? 256u * j : (uint64_t)((256u * j) & ((1u << S) - 1u)) | ((uint64_t)(j >> (S - 8u)) << first);
            a[j] = __builtin_nontemporal_load(p + o);
        }
    };
    // (the counter's partial sums of row k are thread k's own words in LDS: in registers they cost the two-qubit exchange
    // shape its second workgroup on a CU)
    __shared__ double stack[QCX_RDM_MAX_GROUP_BITS * NR];
    uint64_t g = blockIdx.x;
    unsigned ui = 0;                                                 // unit ui of group g
    if (g < ngroups) load(g << ug);
    while (g < ngroups) {
        const uint64_t g_next = ui + 1u == (1u << ug) ? g + gridDim.x : g;
        const unsigned ui_next = ui + 1u == (1u << ug) ? 0u : ui + 1u;
        const bool more = g_next < ngroups;
        const uint64_t u_next = (g_next << ug) + ui_next;
        amp_t x[EPT];
        if constexpr (EXCH) {
#pragma unroll
            for (unsigned j = 0; j < EPT; j++) sa[amp_pos(tid + 256u * j)] = a[j];
            __syncthreads();
            if (more) load(u_next);
            const unsigned fm = (1u << first) - 1u;
#pragma unroll
            for (unsigned j = 0; j < EPT; j++) {
                const unsigned ep = tid + 256u * j, r = ep & ((1u << S) - 1u), v = ep >> S;
                x[j] = sa[amp_pos((r & fm) | (v << first) | ((r >> first) << (first + NUM)))];
            }
        } else {
#pragma unroll
            for (unsigned j = 0; j < EPT; j++) x[j] = a[j];
            if (more) load(u_next);
        }
#pragma unroll
        for (unsigned gr = 0; gr < NG; gr++) {
            double v[GROUP];
#pragma unroll
            for (unsigned i = 0; i < GROUP; i++) {
                const unsigned I = gr * GROUP + i, c = I / NR, row = I % NR, rv = row / NV, rw = row % NV;
                if (rv <= rw) {
                    const amp_t p = x[rv * C + c], q = x[rw * C + c];
                    v[i] = p.x * q.x + p.y * q.y;
                } else {
                    const amp_t p = x[rw * C + c], q = x[rv * C + c];
                    v[i] = p.y * q.x - p.x * q.y;
                }
            }
#pragma unroll
            for (unsigned l = 0; l < HL; l++) {
                const unsigned half = GROUP >> (l + 1u);
                const bool up = ((lane >> l) & 1u) != 0;
#pragma unroll
                for (unsigned i = 0; i < half; i++) {
                    const double keep = up ? v[i + half] : v[i], send = up ? v[i] : v[i + half];
                    v[i] = keep + rdm_xor_lane(send, l);
                }
            }
#pragma unroll
            for (unsigned l = HL; l < 6u; l++) v[0] = v[0] + rdm_xor_lane(v[0], l);
            if ((lane >> HL) == 0) ws[wave * NVAL + gr * GROUP + held] = v[0];
        }
        __syncthreads();
        if (tid < NR) {
            double s[C];
#pragma unroll
            for (unsigned c = 0; c < C; c++) {
                const double *w = ws + c * NR + tid;
                s[c] = (w[0] + w[NVAL]) + (w[2u * NVAL] + w[3u * NVAL]);
            }
#pragma unroll
            for (unsigned len = C; len > 1u; len >>= 1)
#pragma unroll
                for (unsigned i = 0; i < len / 2u; i++) s[i] = s[2u * i] + s[2u * i + 1u];
            // the unit's root joins the group's tree (ui is the same for all threads)
            double root = 0.0 + s[0];
            bool carry = true;
#pragma unroll
            for (unsigned l = 0; l < QCX_RDM_MAX_GROUP_BITS; l++)
                if (carry && l < ug) {
                    if ((ui >> l) & 1u) root = stack[l * NR + tid] + root;
                    else { stack[l * NR + tid] = root; carry = false; }
                }
            if (carry) dst[tid * row_stride + g] = root;             // (every bit of ui set: the group's last unit)
        }
        // (EXCH: the next unit writes sa, which all have read, and ws only behind its own first barrier)
        if constexpr (!EXCH) __syncthreads();
        g = g_next; ui = ui_next;
    }
}

__global__ __launch_bounds__(256) void k_rdm_small(const amp_t *__restrict__ amp, double *__restrict__ dst, unsigned n, unsigned first,
                                                   unsigned num)
{
    __shared__ amp_t sa[2048];
    __shared__ double red[4096];
    const unsigned tid = threadIdx.x, nel = 1u << n, S = n - num, NV = 1u << num, fm = (1u << first) - 1u;
    for (unsigned e = tid; e < nel; e += 256u) sa[e] = amp[e];
    __syncthreads();
    const unsigned total = (NV * NV) << S, batch = total < 4096u ? total : 4096u;      // (a batch holds whole rows: S <= 11)
    for (unsigned b0 = 0; b0 < total; b0 += batch) {
        for (unsigned k = tid; k < batch; k += 256u) {
            const unsigned row = (b0 + k) >> S, r = (b0 + k) & ((1u << S) - 1u), rv = row >> num, rw = row & (NV - 1u);
            const unsigned base = (r & fm) | ((r >> first) << (first + num));
            const amp_t p = sa[base | ((rv <= rw ? rv : rw) << first)], q = sa[base | ((rv <= rw ? rw : rv) << first)];
            red[k] = rv <= rw ? p.x * q.x + p.y * q.y : p.y * q.x - p.x * q.y;
        }
        __syncthreads();
        // the tree levels of every row of the batch, lowest summed bit first; in place (read all, barrier, write all)
        unsigned sz = batch;
        for (unsigned h = 0; h < S; h++) {
            const unsigned half = sz >> 1;
            double v[8];
#pragma unroll
            for (unsigned m = 0; m < 8u; m++) {
                const unsigned k = tid + 256u * m;
                if (k < half) v[m] = red[2u * k] + red[2u * k + 1u];
            }
            __syncthreads();
#pragma unroll
            for (unsigned m = 0; m < 8u; m++) {
                const unsigned k = tid + 256u * m;
                if (k < half) red[k] = v[m];
            }
            __syncthreads();
            sz = half;
        }
        for (unsigned k = tid; k < sz; k += 256u) dst[(b0 >> S) + k] = 0.0 + red[k];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// K18  a diagonal operator on the qubit range [first, first + num) from a table (qcx_diagonal_gate, DESIGN s4.5n;
// tests/diagonal_ref.py is the definition): amp[i] = q_row(tab[k(i)] * amp[i]), k(i) = (i >> first) & kmask, kmask = 2^num - 1,
// the product by q_mul (the pinned arithmetic), zero components multiplied out.  This is K15 SHAPE 0 with the entry taken from
// memory instead of (c, -+s) by parity: the same tiles (T = min(n, 12) lowest index bits, a workgroup of 256 threads, element
// e = tid + 256 j, j < 16), at most 8 amplitudes of a thread in flight, no barrier in the walk, nontemporal loads and stores of
// the state; the table is read with ordinary loads (it is the one thing here that is used again).  Every amplitude is rewritten
// as 0 + ..., so a result is never -0, and an Inf or NaN stays in its own row: there is no strict twin.
// Where the entry comes from (qcx_diagonal_plan in include/qcx_plan.h is the rule; i = (u << T) | e throughout, in 64 bits):
//   FORM 0  num == 0 or first >= T: one entry per tile, k = ((u << T) >> first) & kmask -- uniform, read once per tile
//   FORM 1  8 <= first < T: the entry depends on j and the tile, not on the lane -- uniform addresses, at most 16 per tile
//   FORM 2  first < 8: an entry per lane.  LDS: the tile's slice of the table is the same for every tile (first + num <= 12) and
//           the workgroup copies its 2^num entries into LDS once; otherwise each lane reads tab[k(i)] itself, contiguous or
//           broadcast 16-B reads that L2 serves
// FULL as in K15: !FULL is the one partial tile of n < 12, where a thread owns the elements with tid + 256 j < 2^T.
// ---------------------------------------------------------------------------
template <int FORM, bool FULL, bool LDS>
__global__ __launch_bounds__(256) void k_diagonal(amp_t *__restrict__ amp, const amp_t *__restrict__ tab, uint64_t nunits, unsigned T,
                                                  unsigned first, uint64_t kmask)
{
    constexpr unsigned EPT = 16u, HALF = 8u;
    static_assert(!LDS || FORM == 2, "only the per-lane form stages its slice");
    extern __shared__ amp_t diag_sd[];
    const unsigned tid = threadIdx.x;
    unsigned nld = EPT;
    if constexpr (!FULL) {
        nld = 0;
#pragma unroll
        for (unsigned j = 0; j < EPT; j++)
            if (tid + 256u * j < (1u << T)) nld = j + 1;
    }
    if constexpr (LDS) {
        for (uint64_t k = tid; k <= kmask; k += 256u) diag_sd[k] = tab[k];
        __syncthreads();
    }
    for (uint64_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const uint64_t base = u << T;
        amp_t *pa = amp + base + tid;
        amp_t m_tile = {0.0, 0.0};
        if constexpr (FORM == 0) m_tile = tab[(base >> first) & kmask];
#pragma unroll 1
        for (unsigned h = 0; h < EPT; h += HALF) {
            amp_t a[HALF], m[HALF];
#pragma unroll
            for (unsigned k = 0; k < HALF; k++)
                if (FULL || h + k < nld) {
                    a[k] = __builtin_nontemporal_load(pa + 256u * (h + k));
                    if constexpr (FORM == 0) m[k] = m_tile;
                    else if constexpr (FORM == 1) m[k] = tab[((base | (uint64_t)(256u * (h + k))) >> first) & kmask];
                    else if constexpr (LDS) m[k] = diag_sd[((tid | (256u * (h + k))) >> first) & (unsigned)kmask];
                    else m[k] = tab[((base | (uint64_t)(tid | (256u * (h + k)))) >> first) & kmask];
                }
#pragma unroll
            for (unsigned k = 0; k < HALF; k++)
                if (FULL || h + k < nld)
                    __builtin_nontemporal_store(q_row(q_mul(m[k].x, m[k].y, a[k])), pa + 256u * (h + k));
        }
    }
}

// the matrices' rule for a table in device memory (qcx_diagonal_gate_device): does tab[0 .. count) hold a component that is not
// finite or exceeds 1 in magnitude?  k_scan_nonfinite with that bound; one read of the table
__global__ __launch_bounds__(256) void k_diag_scan(const amp_t *__restrict__ tab, uint64_t count, unsigned *flag)
{
    bool bad = false;
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < count; k += (uint64_t)gridDim.x * 256u) {
        const amp_t v = tab[k];
        bad |= !(fabs(v.x) <= 1.0) || !(fabs(v.y) <= 1.0);
    }
    if (__ballot(bad) && (threadIdx.x & 63u) == 0u) atomicOr(flag, 1u);
}

// ---------------------------------------------------------------------------
// K19  a permutation of the basis states of the qubit range [first, first + num), num <= 12, from a table, under any control
// mask (qcx_permutation_gate, DESIGN s4.5o; tests/permutation_ref.py is the definition): where (i & ctrl_mask) == ctrl_values,
//     new[i] = old[i with its range field k replaced by inv[k]],   inv = the inverse of the caller's table,
// in place, k_camodc's way: a tile of 2^T amplitudes that is closed under the table is staged in LDS with coalesced loads, and
// after the barrier every element fetches its source out of LDS and goes to its OWN address, so the stores are coalesced too
// and no workgroup reads what another writes.  qcx_permutation_plan (include/qcx_plan.h) is the rule; in the kernel's terms:
//   tile_mask  the T index bits of a tile: the num range bits and the lowest T - num other bits that are not squeezed; tile
//              element e stands for the offset deposit(e, tile_mask) -- its low bits are the tile's low bits, so consecutive
//              threads touch consecutive amplitudes in runs as long as the tile's lowest run of bits
//   unit_mask  the index bits that number the tiles: base(u) = deposit(u, unit_mask) | orc, orc = the positive squeezed controls
//              (K17's rule: a control at bit >= 3 is squeezed out, the part of the state where it does not fire is never read)
//   pmask, pvals  the controls that are NOT squeezed (those below bit 3; STRICT: all of them), a predicate on the index: the
//              part inside the tile is tested per element, the part outside it per tile -- a tile that misses is skipped
//   pf         where the range field sits in e: src(e) = e with (e >> pf) & kmask replaced by inv[...]
// deposit is bit-wise and the block a power of two, so deposit(tid + B j) = deposit(tid) | deposit(B j): the first part is
// formed once per thread, the second once per workgroup (joff, 128 B of static LDS, read at a uniform address) -- formed per
// element, the bit loop made the kernel ALU-bound (n = 30: 9.5 ms a pass at every tile size).  The gathered LDS read is a 16-B read per lane: the 16 lanes of a read group
// take 16 different slots of a bank row whenever pf >= 4 (they differ in e's low four bits alone); with the range lower than
// that the slots are the table's and some reads serialise.  Elements that do not fire keep their bits: they are not stored, or
// with store_all stored back as read so that whole lines leave.
// STRICT is the pass of a register flagged non-finite: nothing squeezed, and EVERY amplitude rewritten through the reference's
// row q_row((1, 0) * x), firing or not, `one` and `z` being kernel arguments so that no product is folded (k_strict_mcu's rule).
// ---------------------------------------------------------------------------
struct PermParams {
    uint64_t tile_mask, unit_mask, orc, pmask, pvals, units;
    unsigned T, pf, num;
    int      store_all;
};

__device__ __forceinline__ uint64_t perm_deposit(uint64_t v, uint64_t mask)
{
    uint64_t r = 0;
    for (; v != 0 && mask != 0; v >>= 1, mask &= mask - 1)
        if (v & 1u) r |= mask & (0 - mask);
    return r;
}

template <bool STRICT, bool NT>
__global__ __launch_bounds__(1024) void k_perm_tile(amp_t *__restrict__ amp, const unsigned short *__restrict__ inv_dev, PermParams P,
                                                    double one, double z)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char qcx_lds_raw[];
    amp_t *tile = reinterpret_cast<amp_t *>(qcx_lds_raw);
    const unsigned TS = 1u << P.T, kmask = (1u << P.num) - 1u, B = blockDim.x, tid = threadIdx.x;
    unsigned short *inv = reinterpret_cast<unsigned short *>(tile + TS);
    __shared__ uint64_t joff[16];                              // deposit(B j): the part of an element's offset that its round j adds
    for (unsigned k = tid; k <= kmask; k += B) inv[k] = inv_dev[k];
    if (tid < 16u) joff[tid] = perm_deposit((uint64_t)tid * B, P.tile_mask);      // (B >= 256 and TS <= 2^12: at most 16 rounds)
    const uint64_t lane_off = perm_deposit(tid, P.tile_mask);
    __syncthreads();
    const uint64_t pe_mask = P.pmask & P.tile_mask, pe_vals = P.pvals & P.tile_mask, pt_mask = P.pmask & ~P.tile_mask, pt_vals = P.pvals & ~P.tile_mask;
    for (uint64_t u = blockIdx.x; u < P.units; u += gridDim.x) {
        const uint64_t base = perm_deposit(u, P.unit_mask) | P.orc;
        const bool tile_fires = (base & pt_mask) == pt_vals;
        if (!STRICT && !tile_fires) continue;                  // (uniform: the whole workgroup skips the tile and its barriers)
        amp_t *g = amp + base;
        for (unsigned e = tid, j = 0; e < TS; e += B, j++) tile[e] = g[lane_off | joff[j]];
        __syncthreads();
        for (unsigned e = tid, j = 0; e < TS; e += B, j++) {
            const uint64_t off = lane_off | joff[j];
            const bool fires = tile_fires && (off & pe_mask) == pe_vals;
            unsigned src = e;
            if (fires) src = (e & ~(kmask << P.pf)) | ((unsigned)inv[(e >> P.pf) & kmask] << P.pf);
            const amp_t v = tile[src];
            if constexpr (STRICT) g[off] = q_row(q_mul(one, z, v));
            else if (fires || P.store_all) st<NT>(g + off, v);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// K20  a dense 2^K x 2^K matrix on K = 1 .. 5 target qubits under any control mask (qcx_mc_multi_qubit_gate, DESIGN s4.5p;
// tests/multi_qubit_ref.py is the definition): where (i & ctrl_mask) == ctrl_values, the 2^K amplitudes x_c of i's group (c
// ascending with the state index) become
//     new_r = q_row(m[r][0] * x_0, m[r][1] * x_1, ...),   products by q_mul (the pinned arithmetic), as a loop,
// m = the caller's matrix permuted to ascending order on the host.  The geometry is K19's with the target set in place of the
// range: a tile of 2^T amplitudes chosen by tile_mask holds every target bit, so it is closed under the operator; it is staged
// in LDS with coalesced loads, computed on, and stored from LDS with every element going to its own address.
//   work       a work item is one group and R = 4 of its rows (2 for K = 1): item = chunk * 2^(T-K) + group, so that the lanes of
//              a wave hold consecutive groups and ONE chunk whenever a tile has 64 groups or more.  The item reads the group's
//              x_c out of LDS in ascending c, once for its R rows, and runs R accumulator chains side by side.
//   matrix     mt[2 (c 2^K + r)] = m[r][c] (re, im), column-major, in device memory: the R entries of a column that an item
//              needs are 16 R contiguous bytes at an address that is uniform over the item's lanes.  The lanes are taken chunk
//              by chunk (readfirstlane; one round where the wave holds one chunk), so the address is provably uniform and the
//              entries come as scalar loads into SGPRs -- no per-lane gather, no LDS for the matrix, and the VGPRs hold the
//              2 R sums, one x and addresses only.
//   in place   the rows stay in registers until every item of the workgroup has read its inputs (a barrier), go to the
//              outputs' slots in LDS, and after a second barrier the tile leaves as it came.
//   slots      element e lives in slot e ^ ((e >> 4) & 15), a permutation inside each 256-B bank row of sixteen 16-B slots:
//              staging and storing stay conflict-free, and the group reads of targets below element bit 4 (lanes 128 B
//              apart for targets 0-2) spread over the row's slots, not over two of them.
//   controls   at bit >= 3 they are squeezed out of the tile numbering (orc holds the positive ones); below bit 3 they lie inside
//              every tile (a tile holds the lowest 12 - K >= 7 other bits) and are a predicate per group, pe_mask / pe_vals on
//              the element's offset.  Groups that do not fire keep their bits: not stored, or with store_all stored as read.
// ---------------------------------------------------------------------------
struct MultiParams {
    uint64_t tile_mask, unit_mask, orc, units;
    unsigned pe_mask, pe_vals;         // the controls below bit 3, as bits of the state index
    unsigned T;
    unsigned emask;                    // the K target bits of a tile element
    int      store_all;
};

__device__ __forceinline__ unsigned multi_slot(unsigned e) { return e ^ ((e >> 4) & 15u); }

// R rows of one group: out[k] = row R chunk + k.  chunk is uniform over the active lanes (the caller sees to it).
template <unsigned K, unsigned R>
__device__ __forceinline__ void multi_rows(const amp_t *tile, const unsigned *tdep, const double *__restrict__ mt, unsigned chunk, unsigned eb,
                                           amp_t (&out)[R])
{
    constexpr unsigned D = 1u << K;
    // (the constant address space: with a uniform address the entries are scalar loads even though the kernel stores to amp)
    typedef const double __attribute__((address_space(4))) *const_doubles;
    const uint64_t at = (uint64_t)(mt + 2u * R * chunk);       // (made uniform HERE: the compiler puts the lanes' own chunk in the caller's place)
    const unsigned at_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(at >> 32)), at_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)at);
    const const_doubles mc = (const_doubles)(((uint64_t)at_hi << 32) | (uint64_t)at_lo);      // (unsigned halves: the builtin returns an int)
#pragma unroll
    for (unsigned k = 0; k < R; k++) { out[k].x = 0.0; out[k].y = 0.0; }
#pragma unroll 8
    for (unsigned c = 0; c < D; c++) {
        const amp_t x = tile[multi_slot(eb | tdep[c])];
        const const_doubles m = mc + 2u * D * c;
#pragma unroll
        for (unsigned k = 0; k < R; k++) {
            const q_mul p(m[2u * k], m[2u * k + 1u], x);
            out[k].x = out[k].x + p.re();
            out[k].y = out[k].y + p.im();
        }
    }
}

template <unsigned K, bool NT>
__global__ __launch_bounds__(1024) void k_multi_tile(amp_t *__restrict__ amp, const double *__restrict__ mt, MultiParams P)
{
    constexpr unsigned D = 1u << K, R = K == 1 ? 2 : 4, NI = K == 1 ? 2 : 1;      // (K = 1: 2^11 items of a 2^12 tile, two per thread)
    extern __shared__ __attribute__((aligned(16))) unsigned char qcx_lds_raw[];
    amp_t *tile = reinterpret_cast<amp_t *>(qcx_lds_raw);
    __shared__ uint64_t joff[16];                              // deposit(B j), k_perm_tile's
    __shared__ unsigned tdep[D];                               // deposit(c, emask): member c of a group, as element bits
    const unsigned TS = 1u << P.T, B = blockDim.x, tid = threadIdx.x;
    if (tid < 16u) joff[tid] = perm_deposit((uint64_t)tid * B, P.tile_mask);
    if (tid < D) tdep[tid] = (unsigned)perm_deposit(tid, P.emask);
    const uint64_t lane_off = perm_deposit(tid, P.tile_mask);
    const unsigned glog = P.T - K, items = TS / R;
    unsigned eb[NI], chunk[NI];
    bool fires[NI];
#pragma unroll
    for (unsigned j = 0; j < NI; j++) {
        const unsigned it = tid + B * j;
        chunk[j] = it >> glog;
        eb[j] = (unsigned)perm_deposit(it & ((1u << glog) - 1u), (TS - 1u) & ~P.emask);
        fires[j] = it < items && ((unsigned)perm_deposit(eb[j], P.tile_mask) & P.pe_mask) == P.pe_vals;
    }
    __syncthreads();
    for (uint64_t u = blockIdx.x; u < P.units; u += gridDim.x) {
        amp_t *g = amp + (perm_deposit(u, P.unit_mask) | P.orc);
        for (unsigned e = tid, j = 0; e < TS; e += B, j++) tile[multi_slot(e)] = g[lane_off | joff[j]];
        __syncthreads();
        amp_t out[NI][R];
#pragma unroll
        for (unsigned j = 0; j < NI; j++) {
            if (!fires[j]) continue;
            for (;;) {                                         // the lanes of one chunk at a time: its rows' entries are scalar loads
                const unsigned cu = __builtin_amdgcn_readfirstlane(chunk[j]);
                if (cu == chunk[j]) { multi_rows<K, R>(tile, tdep, mt, cu, eb[j], out[j]); break; }
            }
        }
        __syncthreads();                                       // (every input has been read)
#pragma unroll
        for (unsigned j = 0; j < NI; j++) {
            if (!fires[j]) continue;
#pragma unroll
            for (unsigned k = 0; k < R; k++) tile[multi_slot(eb[j] | tdep[R * chunk[j] + k])] = out[j][k];
        }
        __syncthreads();
        for (unsigned e = tid, j = 0; e < TS; e += B, j++) {
            const uint64_t off = lane_off | joff[j];
            if (P.store_all || ((unsigned)off & P.pe_mask) == P.pe_vals) st<NT>(g + off, tile[multi_slot(e)]);
        }
        __syncthreads();
    }
}

// K20s  the same operator as a STRICT pass (K9's reason: a register that holds non-finite amplitudes): nothing squeezed, one
// thread per group with the group's inputs in registers, the defined rows where (i & cmask) == cvals and every other amplitude
// rewritten through the reference's identity row q_row((1, 0) * x); `one` and `z` are kernel arguments so that no product is
// folded (k_strict_mcu's rule).  tq: the targets in ascending order.
struct MultiTargets { unsigned char q[5]; };

template <unsigned K>
__global__ __launch_bounds__(256) void k_strict_multi(amp_t *__restrict__ amp, unsigned n, MultiTargets tq, uint64_t cmask, uint64_t cvals,
                                                      const double *__restrict__ mt, double one, double z)
{
    constexpr unsigned D = 1u << K;
    const uint64_t groups = (uint64_t)1 << (n - K);
    for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < groups; p += (uint64_t)gridDim.x * 256u) {
        uint64_t i = p;
#pragma unroll
        for (unsigned j = 0; j < K; j++) i = insert_zero(i, tq.q[j]);
        uint64_t bit[K];
#pragma unroll
        for (unsigned j = 0; j < K; j++) bit[j] = (uint64_t)1 << tq.q[j];
        const auto dep = [&](unsigned c) {                     // member c of the group (c is a constant of the unrolled loops)
            uint64_t d = 0;
#pragma unroll
            for (unsigned j = 0; j < K; j++) if ((c >> j) & 1u) d |= bit[j];
            return d;
        };
        amp_t x[D];
#pragma unroll
        for (unsigned c = 0; c < D; c++) x[c] = amp[i | dep(c)];
        if ((i & cmask) == cvals) {
#pragma unroll
            for (unsigned r = 0; r < D; r++) {
                amp_t acc = q_row();
#pragma unroll
                for (unsigned c = 0; c < D; c++) {
                    const q_mul pr(mt[2u * (c * D + r)], mt[2u * (c * D + r) + 1u], x[c]);
                    acc.x = acc.x + pr.re();
                    acc.y = acc.y + pr.im();
                }
                amp[i | dep(r)] = acc;
            }
        } else {
#pragma unroll
            for (unsigned c = 0; c < D; c++) amp[i | dep(c)] = q_row(q_mul(one, z, x[c]));
        }
    }
}

}  // namespace qcx
