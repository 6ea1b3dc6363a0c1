#!/usr/bin/env python3
"""How accurate the TOLERANCE MODE (qcx_set_fusion(reg, 2)) is, measured: every circuit of tests/test_gpu_tolerance_mode.py up to
n = 20, the run-merge edges, the n = 28 inverse QFT on basis states (windows) and the prefixes of tests/tolerance_twin.py, each on
the GPU against the extended-precision truth of tests/exact_ref.py, next to the oracle's own error against that truth.  Needs a
GPU, takes no arguments, writes profiles/tolerance_accuracy.jsonl, one line per case:

    e_oracle_max, e_oracle_l2     the oracle's relative error against the truth (max norm / largest amplitude; 2-norm)
    e_mode2_max, e_mode2_l2       the same of the state the GPU left
    ratio_max, ratio_l2           e_mode2 / max(e_oracle, 2^-52): what exact_ref.assert_as_accurate_as_oracle bounds by MARGIN
    diag_passes                   fused passes that carried merged diagonals (qcx_diag_stats)
    emu_ratio_max, emu_ratio_l2   the same ratios of tests/fuse_emulator.py on qcx_fusion_plan(mode 2) under the same knobs
                                  (null where a case has no such plan: circuits behind a reset run compact chains on the GPU)

    python tools/measure_tolerance_accuracy.py
"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import quantumcomputer_amd as qc                    # noqa: E402
from oracle import binding as ob                    # noqa: E402
import exact_ref as er                              # noqa: E402
import fuse_emulator as emu                         # noqa: E402
import sequence_replay as sr                        # noqa: E402
import tolerance_cases as tc                        # noqa: E402
import tolerance_twin as tt                         # noqa: E402

KNOB_KEYS = sorted({"fuse_T", "fuse_c", "fuse_grid_cap", "fuse_T_phase", "fuse_c_phase", "fuse_phase_ratio", "fuse_tol_occ", "fuse_hsweep_T",
                    "fuse_tol_T", "fuse_q3", "fuse_x8t"} | set(tc.EDGE_KNOB_KEYS))
W = 13


def descs_of(steps):
    out = []
    for s in steps:
        if s[0] == "h":
            out.append((0, s[1], 0, 0.0, 0.0, 0, 0))
        elif s[0] == "p":
            c, sn = qc.polar(s[3])
            out.append((1, 0, (1 << s[1]) | (1 << s[2]), c, sn, 0, 0))
        else:
            out.append((2, s[3], 0, 0.0, 0.0, s[1], s[2] % s[1]))
    return out


def emulated(start, n, M, steps):
    descs = descs_of(steps)
    acts, recs, _ = qc.fusion_plan(n, M, descs, mode=2)
    state = np.array(start)
    emu.run_plan(state, n, M, descs, acts, recs, ob)
    return state


class Out:
    def __init__(self, path):
        self.f = open(path, "w")
        self.worst = (0.0, None)

    def row(self, case, fig, diag_passes, emu_fig=None, **more):
        r = dict(case=case, **{k: float(f"{v:.4g}") for k, v in fig.items()}, diag_passes=diag_passes,
                 emu_ratio_max=None if emu_fig is None else float(f"{emu_fig['ratio_max']:.4g}"),
                 emu_ratio_l2=None if emu_fig is None else float(f"{emu_fig['ratio_l2']:.4g}"), **more)
        self.f.write(json.dumps(r) + "\n"); self.f.flush()
        print(json.dumps(r), flush=True)
        self.worst = max(self.worst, (max(fig["ratio_max"], fig["ratio_l2"]), case))


def run_steps(n, M, start_call, steps):
    """(state, passes with merged diagonals) of a fresh register in mode 2"""
    with qc.Register(n - M, M) as reg:
        reg.set_fusion(2)
        start_call(reg)
        d0 = sr.diagonal_passes(qc, reg)
        tc.apply_steps(qc, reg, steps)
        got = reg.read()
        return got, sr.diagonal_passes(qc, reg) - d0


def main():
    qc.lib(); ob.lib()
    old = {k: qc.lib().qcx_tune_get(k.encode()) for k in KNOB_KEYS}
    out = Out(os.path.join(ROOT, "profiles", "tolerance_accuracy.jsonl"))

    def case(name, n, M, start_call, start, steps, want, truth, knobs, emulate=True, halves=None):
        qc.tune(**old); qc.tune(**knobs)
        got, dp = run_steps(n, M, start_call, steps)
        e = emulated(start, n, M, steps) if emulate else None
        out.row(name, er.figures(got, want, truth), dp, None if e is None else er.figures(e, want, truth), n=n, M=M, knobs=knobs)
        for hname, where in (halves or {}).items():
            out.row(f"{name}: half-space of the {hname} factor", er.figures(got, want, truth, where), dp, er.figures(e, want, truth, where), n=n, M=M, knobs=knobs)

    try:
        for n, M in tc.IQFT_SHAPES:
            want, truth, _ = tc.iqft_case(ob, n, M, tc.IQFT_SEED)
            for geom, gid in zip(tc.IQFT_GEOMS, tc.IQFT_GEOM_IDS):
                if geom and geom[0] > n:
                    continue
                knobs = dict(fuse_T=geom[0], fuse_c=geom[1], fuse_T_phase=0, fuse_tol_T=0, fuse_q3=0) if geom else {}
                case(f"iqft n={n} M={M} {gid}", n, M, lambda reg: reg.fill_random(tc.IQFT_SEED), ob.fill_random(n, tc.IQFT_SEED), er.iqft_steps(n, M),
                     want, truth, knobs)
        for Cn, L, M, a in tc.SHOR_SHAPES:
            n = L + M
            want, truth, _ = tc.shor_case(ob, Cn, L, M, a)
            for occ in (6, 8):
                qc.tune(**old); qc.tune(fuse_tol_occ=occ)
                with qc.Register(L, M) as reg:
                    reg.set_fusion(2)
                    qc.reset_register(reg)
                    qc.quantum_computation(Cn, a, reg)
                    got, dp = reg.read(), sr.diagonal_passes(qc, reg)
                e = emulated(er.basis_state(n, 1), n, M, er.qcomp_steps(Cn, a, L, M))
                out.row(f"shor C={Cn} L={L} M={M} occ={occ}", er.figures(got, want, truth), dp, er.figures(e, want, truth), n=n, M=M, knobs=dict(fuse_tol_occ=occ))
        for seed in tc.PROGRAM_SEEDS:
            n, M, Cn, knobs, steps = tc.random_program(seed)
            want, truth, _ = tc.program_case(ob, seed)
            case(f"program {seed}", n, M, lambda reg: reg.fill_random(seed), ob.fill_random(n, seed), steps, want, truth, knobs)
        for n, M in tc.RADIX8_SHAPES:
            if n <= tc.RADIX8_TRUTH_MAX_N:
                want, truth, _ = tc.iqft_case(ob, n, M, tc.RADIX8_SEED)
                case(f"radix-8 iqft n={n} M={M}", n, M, lambda reg: reg.fill_random(tc.RADIX8_SEED), ob.fill_random(n, tc.RADIX8_SEED), er.iqft_steps(n, M),
                     want, truth, {})
        want, truth, _ = tc.edge_case(ob)
        for knobs, kid in zip(tc.EDGE_KNOBS, tc.EDGE_KNOB_IDS):
            case(f"edges {kid}", tc.EDGE_N, 0, lambda reg: reg.fill_random(tc.EDGE_SEED), ob.fill_random(tc.EDGE_N, tc.EDGE_SEED), tc.edge_steps(),
                 want, truth, knobs, halves=tc.edge_half_spaces())
        qc.tune(**old)
        # the prefixes of the twin pairs under the default knobs (tests/tolerance_twin.py)
        with tempfile.TemporaryDirectory() as tmp:
            import pathlib
            for kind in tt.PREFIX_KINDS:
                for shape in tt.SHAPES + ([tt.BIG_SHAPE] if kind == "shor" else []):
                    if not tt.prefix_is_legal(kind, shape):
                        continue
                    prefix = tt.prefix_ops(kind, shape)
                    S, stats, chains, _ = tt.run_twin(qc, shape, prefix, pathlib.Path(tmp))
                    out.row(f"twin {tt.key_of(kind, shape)}", er.figures(S, tt.oracle_state(ob, kind, shape)[0], tt.truth_of(ob, shape, prefix)), stats[2],
                            n=shape[0] + shape[1], M=shape[1], knobs={}, compact_chains=chains)
        # n = 28 on basis states: the worst window of each input
        n = 28
        rs = np.random.RandomState(29)
        with qc.Register(n, 0) as reg:
            reg.set_fusion(2)
            for x in (0, (1 << n) - 1, 0x5A5A5A5 & ((1 << n) - 1), (1 << (n - 1)) | 1):
                qc.reset_register(reg)
                if x != 1:
                    reg.write(np.array([0.0, 0.0]), first=1)
                    reg.write(np.array([1.0, 0.0]), first=x)
                d0 = sr.diagonal_passes(qc, reg)
                qc.inverse_QFT(reg)
                starts = {0, (1 << n) - (1 << W), x & ~((1 << W) - 1)} | {int(v) << W for v in rs.randint(0, 1 << (n - W), 4)}
                figs = [er.figures(reg.read(s, 1 << W), ob.basis_iqft_window(x, n, 0, s, 1 << W), er.basis_iqft_window(x, n, 0, s, 1 << W)) for s in sorted(starts)]
                worst = max(figs, key=lambda f: max(f["ratio_max"], f["ratio_l2"]))
                out.row(f"iqft n=28 on |{x:#x}>, worst of {len(figs)} windows of 2^{W}", worst, sr.diagonal_passes(qc, reg) - d0, n=n, M=0, knobs={})
    finally:
        qc.tune(**old)
    print(f"worst ratio {out.worst[0]:.3f} ({out.worst[1]}); the criterion allows {er.MARGIN}")


if __name__ == "__main__":
    main()
