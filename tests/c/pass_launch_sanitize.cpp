// The launch plan of a fused pass (pass_launch_plan, csrc/qcx_fuse.inc.h) under AddressSanitizer + UBSan on the host side: a
// stand-alone program around the library's source, no GPU needed (nothing here makes a HIP call).  Build and run:
//   hipcc -O1 -g --offload-arch=gfx950 -ffp-contract=off -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all -o pass_launch_sanitize tests/c/pass_launch_sanitize.cpp && ./pass_launch_sanitize
// It walks a slice of the enumeration of tests/pass_launch_cases.py (every T, dg_slim, dg_cnt, gen and flag; the sizes at their
// extremes) under the default knobs and under a few hostile ones, and checks what must hold of every answer: a named kernel,
// a block the kernel exists for, the areas inside the LDS bytes, or a refusal with its text.
#include "../../quantumcomputer_amd/csrc/qcx_api.hip"

static unsigned long g_ok = 0, g_refused = 0;

static int check(const qcx_pass_launch_in &I)
{
    qcx_pass_launch_out O;
    const int st = qcx_pass_launch_plan(&I, &O);
    if (st != QCX_NO_ERROR) {
        if (st != QCX_UNKNOWN_ERROR || !qcx_last_error()[0] || O.kernel[0]) { fprintf(stderr, "refusal without a text (status %d)\n", st); return 1; }
        g_refused++;
        return 0;
    }
    const size_t front = strstr(O.kernel, "k_gen_cols") ? (size_t)I.zpad * QCX_COL_STRIDE * sizeof(amp_t) : (size_t)16 << I.T;
    const bool bad = !strchr(O.kernel, '<') || O.grid < 1 || O.block < 64 || O.block > 1024 || (O.block & 63u) || O.lds_bytes < front ||
                     front + O.xm_off > O.lds_bytes || front + O.dg_lds_off > O.lds_bytes || front + O.gen_lds_off > O.lds_bytes ||
                     (O.waves != 0) != (strstr(O.kernel, "k_gen_cols") != nullptr) || (O.expanding_store_ok && !strstr(O.kernel, "k_fused_x8<512, 12, false"));
    if (bad) { fprintf(stderr, "bad plan: %s grid %u block %u lds %u (T = %u, dg_slim = %u, gen = %u)\n", O.kernel, O.grid, O.block, O.lds_bytes, I.T, I.dg_slim, I.gen); return 1; }
    g_ok++;
    return 0;
}

int main()
{
    static const struct { const char *key; long value; } knobs[][3] = {
        {{nullptr, 0}}, {{"fuse_ldsdma", 0}, {nullptr, 0}}, {{"fuse_rounds_occ", 0}, {"fuse_x8t", 0}, {nullptr, 0}},
        {{"fuse_streams_log2", 40}, {"fuse_streams_pos", 1000}, {nullptr, 0}}, {{"fuse_cols_waves", 99}, {"fuse_grid_cap", -5}, {nullptr, 0}}};
    for (const auto &set : knobs) {
        g_tune = Tune();
        for (int k = 0; k < 3 && set[k].key; k++) if (qcx_tune_set(set[k].key, set[k].value) != QCX_NO_ERROR) return 2;
        for (unsigned T = 5; T <= 13; T++) for (unsigned slim = 0; slim < 4; slim++) for (unsigned dg : {0u, 3u, 16u, 255u}) for (unsigned gen = 0; gen < 4; gen++)
        for (unsigned flags = 0; flags < 128; flags++) for (unsigned big = 0; big < 2; big++) for (unsigned n : {T, T + 2, 40u}) {
            qcx_pass_launch_in I;
            memset(&I, 0, sizeof I);
            I.n = n; I.M = big ? 26 : 4; I.T = T; I.dg_slim = slim; I.dg_cnt = dg; I.gen = gen;
            I.has_cam = flags & 1; I.rounds_form = (flags >> 1) & 1; I.chained = (flags >> 2) & 1; I.xp_on = (flags >> 3) & 1;
            I.tables_cover = (flags >> 4) & 1; I.buffers_differ = (flags >> 5) & 1; I.zskip = (flags >> 6) & 1 ? 2 : 0;
            I.table_bytes = big ? 4096 : 0; I.xm_cnt = big ? 4000 : 0; I.zpad = big ? 16 : 6; I.gen_tab_bytes = big ? 64 : 0;
            if (check(I)) return 1;
        }
    }
    qcx_pass_launch_in I;
    memset(&I, 0, sizeof I);
    qcx_pass_launch_out O;
    if (qcx_pass_launch_plan(&I, &O) != QCX_BAD_ARGUMENTS || qcx_pass_launch_plan(nullptr, &O) != QCX_BAD_ARGUMENTS) return 3;
    I.n = 10; I.T = 12; I.tables_cover = 1;
    if (qcx_pass_launch_plan(&I, &O) != QCX_UNKNOWN_ERROR) return 3;
    printf("pass_launch_sanitize ok: %lu plans, %lu refusals\n", g_ok, g_refused);
    return g_ok > 1000 && g_refused > 1000 ? 0 : 4;
}
