// The host side of qcx_permutation_gate (csrc/qcx_api.hip: the table's check and inversion, permutation_invert, and the launch
// rule, qcx_permutation_plan) under AddressSanitizer + UBSan: a stand-alone program around the library's source, no GPU needed
// (nothing here makes a HIP call).  Build and run:
//   hipcc -O1 -g --offload-arch=gfx950 -ffp-contract=off -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all -o permutation_sanitize tests/c/permutation_sanitize.cpp && ./permutation_sanitize
// It walks the grid of tests/test_permutation_plan.py -- every range of n = 1 .. 14 and a few of n = 30 .. 40, under no control
// and under controls at bits 0, 2, 3, first - 1, first + num and n - 1 of both polarities --, the plan's refusals, the strict
// form, and tables that are bijections, that repeat a value and that hold a value out of range; the table and its inverse live
// in heap blocks of exactly their size, so a read or write past either end is caught.
#include "../../quantumcomputer_amd/csrc/qcx_api.hip"

#include <memory>
#include <numeric>
#include <random>

static unsigned long g_plans = 0, g_refused = 0, g_tables = 0;

static int check_plan(unsigned n, uint64_t cm, uint64_t cv, unsigned first, unsigned num, bool strict)
{
    qcx_perm_plan pl;
    PermParams P;
    const int st = permutation_plan(tune_now(), n, cm, cv, first, num, strict, &pl, &P);
    if (st != QCX_NO_ERROR) { g_refused++; return 0; }
    const uint64_t nmask = (((uint64_t)1) << n) - 1u;
    const uint64_t sq = strict ? 0 : pl.geom.squeezed;
    bool bad = (pl.geom.tile_mask | pl.geom.unit_mask | sq) != nmask || (pl.geom.tile_mask & pl.geom.unit_mask) != 0 || ((pl.geom.tile_mask | pl.geom.unit_mask) & sq) != 0;
    bad = bad || (unsigned)__builtin_popcountll(pl.geom.tile_mask) != pl.geom.T || pl.geom.T > 12 || pl.range_pos + num > pl.geom.T;
    bad = bad || (pl.geom.units << pl.geom.T) != (((uint64_t)1) << (n - (unsigned)__builtin_popcountll(sq))) || pl.grid < 1 || pl.grid > pl.geom.units;
    bad = bad || pl.lds_bytes > 73728 || (pl.block != 256 && pl.block != 1024) || !strchr(pl.kernel, '<') || pl.geom.nruns > QCX_PERM_MAX_RUNS;
    bad = bad || P.tile_mask != pl.geom.tile_mask || P.unit_mask != pl.geom.unit_mask || P.units != pl.geom.units || P.T != pl.geom.T || P.pf != pl.range_pos;
    bad = bad || (P.pmask & sq) != 0 || (P.pvals & ~P.pmask) != 0 || (P.orc & ~sq) != 0;
    for (unsigned k = 0; k < pl.geom.T; k++) bad = bad || !((pl.geom.tile_mask >> pl.geom.tile_bits[k]) & 1u);
    if (bad) { fprintf(stderr, "bad plan: n %u mask %#llx values %#llx first %u num %u strict %d\n", n, (unsigned long long)cm, (unsigned long long)cv, first, num, (int)strict); return 1; }
    g_plans++;
    return 0;
}

static int check_grid(unsigned n)
{
    for (unsigned first = 0; first <= n; first++)
        for (unsigned num = 0; first + num <= n + 1; num++) {                // (one past the register too: a refusal)
            if (n > 14 && num > 13 && first + num < n) continue;
            const long cand[] = {-1, 0, 2, 3, (long)first - 1, (long)(first + num), (long)n - 1, (long)n};
            for (long c : cand) for (int pol = 0; pol < 2; pol++) for (int strict = 0; strict < 2; strict++) {
                uint64_t cm = 0;
                if (c >= 0 && c < 64) cm = ((uint64_t)1) << c;
                if (check_plan(n, cm, pol ? cm : 0, first, num, strict != 0)) return 1;
            }
            // every qubit outside the range a control, alternating polarity
            uint64_t all = (((uint64_t)1) << n) - 1u;
            if (first + num <= n) all &= ~(((((uint64_t)1) << num) - 1u) << first);
            if (check_plan(n, all, all & 0x5555555555555555ULL, first, num, false) || check_plan(n, all, all & 0xAAAAAAAAAAAAAAAAULL, first, num, true)) return 1;
        }
    return 0;
}

static int check_tables()
{
    std::mt19937 rng(12345);
    for (unsigned num = 0; num <= QCX_PERM_MAX_QUBITS; num++) {
        const uint32_t entries = 1u << num;
        std::unique_ptr<uint32_t[]> perm(new uint32_t[entries]);
        std::unique_ptr<uint16_t[]> inv(new uint16_t[entries]);
        unsigned long moved = 99;
        std::iota(perm.get(), perm.get() + entries, 0u);
        if (permutation_invert(num, perm.get(), inv.get(), &moved) != QCX_NO_ERROR || moved != 0) return 1;
        for (int rep = 0; rep < 4; rep++) {
            std::shuffle(perm.get(), perm.get() + entries, rng);
            if (permutation_invert(num, perm.get(), inv.get(), &moved) != QCX_NO_ERROR) return 1;
            unsigned long want = 0;
            for (uint32_t k = 0; k < entries; k++) { if (inv[perm[k]] != k) return 1; want += perm[k] != k; }
            if (moved != want) return 1;
            g_tables++;
        }
        if (num == 0) {
            perm[0] = 1;
            if (permutation_invert(num, perm.get(), inv.get(), &moved) != QCX_BAD_ARGUMENTS || !strstr(qcx_last_error(), "entry 0 is 1")) return 2;
            continue;
        }
        // a value repeated: the later of the two entries is named; a value out of range, by one and by far
        const uint32_t a = rng() % entries, b = (a + 1 + rng() % (entries - 1)) % entries, lo = a < b ? a : b, hi = a < b ? b : a;
        const uint32_t keep = perm[hi];
        perm[hi] = perm[lo];
        char want[64];
        snprintf(want, sizeof want, "entry %u is %u,", hi, perm[hi]);
        if (permutation_invert(num, perm.get(), inv.get(), &moved) != QCX_BAD_ARGUMENTS || !strstr(qcx_last_error(), want) || !strstr(qcx_last_error(), "bijection")) return 2;
        perm[hi] = keep;
        for (uint32_t v : {entries, 0xFFFFu, 0x10000u, 0xFFFFFFFFu}) {
            if (v < entries) continue;
            const uint32_t k = rng() % entries, was = perm[k];
            perm[k] = v;
            snprintf(want, sizeof want, "entry %u is %u,", k, v);
            if (permutation_invert(num, perm.get(), inv.get(), &moved) != QCX_BAD_ARGUMENTS || !strstr(qcx_last_error(), want)) return 2;
            perm[k] = was;
            g_tables++;
        }
    }
    return 0;
}

int main()
{
    static const struct { const char *key; long value; } knobs[][3] = {
        {{nullptr, 0}}, {{"perm_grid_cap", 0}, {nullptr, 0}}, {{"perm_grid_cap", -7}, {"perm_store_all", 0}, {nullptr, 0}}, {{"perm_nt", 5}, {"perm_grid_cap", 3}, {nullptr, 0}},
        {{"perm_tile_log2", 8}, {nullptr, 0}}, {{"perm_tile_log2", -3}, {"perm_grid_cap", 1}, {nullptr, 0}}, {{"perm_tile_log2", 99}, {nullptr, 0}}};
    for (const auto &set : knobs) {
        g_tune = Tune();
        for (int k = 0; k < 3 && set[k].key; k++) if (qcx_tune_set(set[k].key, set[k].value) != QCX_NO_ERROR) return 2;
        for (unsigned n = 1; n <= 14; n++) if (check_grid(n)) return 1;
        for (unsigned n : {30u, 33u, 34u, 40u}) if (check_grid(n)) return 1;
    }
    qcx_perm_plan pl;
    if (qcx_permutation_plan(0, 0, 0, 0, 0, &pl) != QCX_BAD_ARGUMENTS || qcx_permutation_plan(41, 0, 0, 0, 0, &pl) != QCX_BAD_ARGUMENTS ||
        qcx_permutation_plan(12, 0, 0, 0, 1, nullptr) != QCX_BAD_ARGUMENTS || qcx_permutation_plan(12, 1, 3, 4, 1, &pl) != QCX_BAD_ARGUMENTS ||
        qcx_permutation_plan(12, 0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, &pl) != QCX_BAD_QUBIT || qcx_permutation_plan(12, ~(uint64_t)0, 0, 0, 0, &pl) != QCX_BAD_QUBIT ||
        qcx_permutation_plan(40, 0, 0, 0, 13, &pl) != QCX_BAD_ARGUMENTS) return 3;
    if (int st = check_tables()) return 10 + st;
    printf("permutation_sanitize ok: %lu plans, %lu refusals, %lu tables\n", g_plans, g_refused, g_tables);
    return g_plans > 10000 && g_refused > 1000 && g_tables > 50 ? 0 : 4;
}
