// The host side of qcx_mc_multi_qubit_gate (csrc/qcx_api.hip: the matrix permuted to ascending order, multi_ascending, the
// argument checks and the launch rule, qcx_multi_gate_plan) under AddressSanitizer + UBSan: a stand-alone program around the
// library's source, no GPU needed (nothing here makes a HIP call).  Build and run:
//   hipcc -O1 -g --offload-arch=gfx950 -ffp-contract=off -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all -o multi_gate_sanitize tests/c/multi_gate_sanitize.cpp && ./multi_gate_sanitize
// It walks target sets of 1 .. 5 qubits (and the refused 0 and 6) in ascending and shuffled order on n = 1 .. 14 and a few of
// n = 30 .. 40, under no control, single controls of both polarities and every other qubit a control, under hostile knobs; the
// targets, the matrix and its permuted copy live in heap blocks of exactly their size, so a read or write past either end is
// caught; the permuted matrix is compared with the rule m[r][c] = u[given(r)][given(c)] recomputed here.
#include "../../quantumcomputer_amd/csrc/qcx_api.hip"

#include <algorithm>
#include <memory>
#include <random>

static unsigned long g_plans = 0, g_refused = 0, g_matrices = 0;

static int check_plan(unsigned n, uint64_t cm, uint64_t cv, unsigned k, const unsigned *targets)
{
    qcx_multi_plan pl;
    MultiParams P;
    const int st = multi_plan(tune_now(), n, cm, cv, k, targets, &pl, &P);
    if (st != QCX_NO_ERROR) { g_refused++; return 0; }
    const uint64_t nmask = (((uint64_t)1) << n) - 1u, sq = pl.geom.squeezed;
    uint64_t tmask = 0;
    for (unsigned j = 0; j < k; j++) tmask |= (uint64_t)1 << targets[j];
    bool bad = (pl.geom.tile_mask | pl.geom.unit_mask | sq) != nmask || (pl.geom.tile_mask & pl.geom.unit_mask) != 0 || ((pl.geom.tile_mask | pl.geom.unit_mask) & sq) != 0;
    bad = bad || (unsigned)__builtin_popcountll(pl.geom.tile_mask) != pl.geom.T || pl.geom.T > 12 || pl.geom.T < k || (pl.geom.tile_mask & tmask) != tmask;
    bad = bad || (pl.geom.units << pl.geom.T) != (((uint64_t)1) << (n - (unsigned)__builtin_popcountll(sq))) || pl.grid < 1 || pl.grid > pl.geom.units;
    bad = bad || pl.lds_bytes > 65536 || pl.block < 64 || pl.block > 1024 || (pl.block & (pl.block - 1)) != 0 || !strchr(pl.kernel, '<') || pl.geom.nruns > QCX_PERM_MAX_RUNS;
    bad = bad || (uint64_t)pl.block * pl.rows_per_item * (k == 1 ? 2 : 1) < (((uint64_t)1) << pl.geom.T);
    bad = bad || pl.geom.unit_mask_low != 0 || pl.geom.form != QCX_PERM_LINES;
    bad = bad || P.tile_mask != pl.geom.tile_mask || P.unit_mask != pl.geom.unit_mask || P.units != pl.geom.units || P.T != pl.geom.T || P.pe_mask != pl.geom.elem_mask || P.pe_vals != pl.geom.elem_values;
    bad = bad || (P.orc & ~sq) != 0 || (unsigned)__builtin_popcount(P.emask) != k || P.emask >= (1u << pl.geom.T);
    for (unsigned j = 0; j < pl.geom.T; j++) bad = bad || !((pl.geom.tile_mask >> pl.geom.tile_bits[j]) & 1u);
    for (unsigned j = 0; j < k; j++) bad = bad || pl.geom.tile_bits[pl.target_pos[j]] != targets[j] || !((P.emask >> pl.target_pos[j]) & 1u);
    if (bad) { fprintf(stderr, "bad plan: n %u mask %#llx values %#llx k %u first target %u\n", n, (unsigned long long)cm, (unsigned long long)cv, k, targets[0]); return 1; }
    g_plans++;
    return 0;
}

static int check_matrix_permutation(unsigned k, const unsigned *targets, std::mt19937 &rng)
{
    const unsigned d = 1u << k;
    std::unique_ptr<double[]> u(new double[2u * d * d]), mt(new double[2u * d * d]);
    std::unique_ptr<unsigned char[]> sorted(new unsigned char[k]);
    for (unsigned j = 0; j < 2u * d * d; j++) u[j] = (double)(rng() % 2001u) / 1000.0 - 1.0;
    multi_ascending(k, targets, u.get(), mt.get(), sorted.get());
    for (unsigned j = 0; j + 1 < k; j++) if (sorted[j] >= sorted[j + 1]) return 1;
    for (unsigned r = 0; r < d; r++)
        for (unsigned c = 0; c < d; c++) {
            unsigned gr = 0, gc = 0;                           // the caller's index of ascending index r, c: bit j = the bit of targets[j]'s rank
            for (unsigned j = 0; j < k; j++) {
                unsigned rank = 0;
                for (unsigned i = 0; i < k; i++) rank += targets[i] < targets[j];
                gr |= ((r >> rank) & 1u) << j; gc |= ((c >> rank) & 1u) << j;
            }
            if (mt[2u * (c * d + r)] != u[2u * (gr * d + gc)] || mt[2u * (c * d + r) + 1u] != u[2u * (gr * d + gc) + 1u]) return 1;
        }
    g_matrices++;
    return 0;
}

static int check_grid(unsigned n, std::mt19937 &rng)
{
    for (unsigned k = 0; k <= QCX_MULTI_MAX_TARGETS + 1; k++) {
        for (int rep = 0; rep < 12; rep++) {
            std::unique_ptr<unsigned[]> t(new unsigned[k ? k : 1]);
            // rep 0: the lowest qubits; 1: the highest; 2: one past the register (a refusal); 3: a repeated target; then random sets
            std::vector<unsigned> all(n);
            for (unsigned q = 0; q < n; q++) all[q] = q;
            std::shuffle(all.begin(), all.end(), rng);
            bool valid = k >= 1 && k <= QCX_MULTI_MAX_TARGETS && k <= n;
            for (unsigned j = 0; j < k; j++) t[j] = rep == 0 ? j : rep == 1 ? n - 1 - j : j < n ? all[j] : n + j;
            if (rep == 2 && k) { t[k - 1] = n; valid = false; }
            if (rep == 3 && k >= 2) { t[k - 1] = t[0]; valid = false; }
            if (rep % 2 && rep > 3 && valid) std::sort(t.get(), t.get() + k);
            uint64_t tmask = 0;
            for (unsigned j = 0; j < k; j++) if (t[j] < 64) tmask |= (uint64_t)1 << t[j];
            const long cand[] = {-1, 0, 2, 3, (long)n - 1, (long)n, (long)(rng() % n)};
            for (long c : cand) for (int pol = 0; pol < 2; pol++) {
                uint64_t cm = 0;
                if (c >= 0 && c < 64) cm = ((uint64_t)1) << c;
                if (check_plan(n, cm, pol ? cm : 0, k, t.get())) return 1;
            }
            const uint64_t others = ((((uint64_t)1) << n) - 1u) & ~tmask;
            if (check_plan(n, others, others & 0x5555555555555555ULL, k, t.get()) || check_plan(n, others, others & 0xAAAAAAAAAAAAAAAAULL, k, t.get())) return 1;
            if (valid && check_matrix_permutation(k, t.get(), rng)) { fprintf(stderr, "bad matrix permutation: n %u k %u\n", n, k); return 1; }
        }
    }
    return 0;
}

int main()
{
    std::mt19937 rng(4321);
    static const struct { const char *key; long value; } knobs[][3] = {
        {{nullptr, 0}}, {{"multi_grid_cap", 0}, {nullptr, 0}}, {{"multi_grid_cap", -7}, {"multi_store_all", 0}, {nullptr, 0}}, {{"multi_nt", 5}, {"multi_grid_cap", 3}, {nullptr, 0}},
        {{"multi_generic", 1}, {"perm_tile_log2", 8}, {nullptr, 0}}};
    for (const auto &set : knobs) {
        g_tune = Tune();
        for (int k = 0; k < 3 && set[k].key; k++) if (qcx_tune_set(set[k].key, set[k].value) != QCX_NO_ERROR) return 2;
        for (unsigned n = 1; n <= 14; n++) if (check_grid(n, rng)) return 1;
        for (unsigned n : {30u, 33u, 34u, 40u}) if (check_grid(n, rng)) return 1;
    }
    // the refusals, in the header's order; the gate's own come before a register is looked at
    qcx_multi_plan pl;
    const unsigned t3[3] = {0, 1, 2}, dup[3] = {4, 1, 4};
    double u[128] = {0};
    if (qcx_multi_gate_plan(0, 0, 0, 3, t3, &pl) != QCX_BAD_ARGUMENTS || qcx_multi_gate_plan(41, 0, 0, 3, t3, &pl) != QCX_BAD_ARGUMENTS ||
        qcx_multi_gate_plan(12, 0, 0, 3, t3, nullptr) != QCX_BAD_ARGUMENTS || qcx_multi_gate_plan(12, 0, 0, 3, nullptr, &pl) != QCX_BAD_ARGUMENTS ||
        qcx_multi_gate_plan(12, 1, 3, 0, t3, &pl) != QCX_BAD_ARGUMENTS || !strstr(qcx_last_error(), "1 to 5") ||
        qcx_multi_gate_plan(12, 1, 3, 6, t3, &pl) != QCX_BAD_ARGUMENTS ||
        qcx_multi_gate_plan(12, 8, 24, 3, dup, &pl) != QCX_BAD_ARGUMENTS || !strstr(qcx_last_error(), "ctrl_values") ||
        qcx_multi_gate_plan(12, 0, 0, 3, dup, &pl) != QCX_BAD_QUBIT || qcx_multi_gate_plan(2, 0, 0, 3, t3, &pl) != QCX_BAD_QUBIT ||
        qcx_multi_gate_plan(12, ~(uint64_t)0, 0, 3, t3, &pl) != QCX_BAD_QUBIT || qcx_multi_gate_plan(12, 1, 1, 3, t3, &pl) != QCX_BAD_QUBIT) return 3;
    if (qcx_mc_multi_qubit_gate(0, 0, 3, t3, u, nullptr) != QCX_BAD_ARGUMENTS) return 3;
    printf("multi_gate_sanitize ok: %lu plans, %lu refusals, %lu matrices\n", g_plans, g_refused, g_matrices);
    return g_plans > 10000 && g_refused > 1000 && g_matrices > 500 ? 0 : 4;
}
