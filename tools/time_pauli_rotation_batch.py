#!/usr/bin/env python3
"""Cost of qcx_pauli_rotation_batch (K15b, DESIGN s4.5k) on one GPU, dense fill_random state of n qubits, against the same list
issued term by term through qcx_pauli_rotation (one launch, one read and one write of the state per term) and against the
yardstick hadamard_gate(12), all timed in the same process on the same register.  The lists:
  z32          32 Z-type terms (29 ZZ bonds and Z on three qubits): one pass of diagonal terms, as wide as a pass gets
  zz29         the 29 ZZ bonds of a chain
  bonds_high   XX, YY, ZZ on the bonds (20,21), (21,22), (22,23): one pass over a tile of bits 0-7 and 20-23
  bonds_low    XX, YY, ZZ on the bonds (8,9), (9,10), (10,11): one pass over the 12 lowest index bits
  heisenberg   the whole step, bond by bond: 3 (n - 1) terms
  ising        the ZZ layer, then X on every qubit: 2 n - 1 terms
Each list is a `batch` row and a `term_by_term` row; the two whole steps also give one row per PASS of their plan (the pass's
terms as a list of their own, which plans to the same single pass).  A batch row carries what its passes move and compute:
traffic_tb_per_s = passes * 32 B * 2^n / time, and fp64_issue_fraction = the FP64 wave-instructions per SIMD the terms need (8
per amplitude for a term without X or Y in the tile, 20 for an exchange term; 64 amplitudes to an instruction, --simds SIMDs)
times the measured 2.18 ns each (DESIGN s8), over the time: 1.0 is the issue ceiling.
HIP events on the register's stream around each case.  The cases alternate, `--reps` rounds after a warm-up call of each; the
Hadamard is in every round TWICE, and the two series, identical work, give the run's own spread.  All rows are timed in ONE child
process under `timeout`.  One JSON object per line, on stdout and in --out.

  python tools/time_pauli_rotation_batch.py [--n 30] [--reps 9] [--out profiles/pauli_rotation_batch_n30_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THETA = 0.37
FP64_NS = 2.18


def bonds(qs, letters="XYZ"):
    out = []
    for q in qs:
        both = 3 << q
        out += [({"X": (both, 0), "Y": (both, both), "Z": (0, both)}[c], THETA) for c in letters]
    return out


def lists(n):
    hi = max(0, min(20, n - 4))
    lo = max(0, min(8, n - 4))
    return [("z32", bonds(range(n - 1), "Z")[:29] + [((0, 1 << q), THETA) for q in (0, n // 2, n - 1)]),
            ("zz29", bonds(range(n - 1), "Z")[:29]),
            ("bonds_high", bonds(range(hi, hi + 3))),
            ("bonds_low", bonds(range(lo, lo + 3))),
            ("heisenberg", bonds(range(n - 1))),
            ("ising", bonds(range(n - 1), "Z") + [((1 << q, 0), THETA) for q in range(n)])]


def step(n, reps, out, simds):
    sys.path.insert(0, ROOT)
    import quantumcomputer_amd as qc
    cases = []                                                       # (name, kind, terms, passes)
    for name, terms in lists(n):
        pass_of, passes = qc.pauli_rotation_batch_plan(terms, n)
        cases.append((name, "batch", terms, passes))
        cases.append((name, "term_by_term", terms, None))
        if name in ("heisenberg", "ising"):
            for p in range(len(passes)):
                sub = [t for t, q in zip(terms, pass_of) if q == p]
                assert qc.pauli_rotation_batch_plan(sub, n)[1] == [passes[p]]
                cases.append((f"{name}_pass_{p}", "batch", sub, [passes[p]]))
    rows = []
    with qc.Register(n, 0) as reg:
        reg.fill_random(30)
        reg.synchronize()
        yard = min(12, n - 1)

        def hadamard():
            qc.hadamard_gate(yard, reg)

        def batch(terms):
            return lambda: qc.pauli_rotation_batch(terms, reg)

        def loop(terms):
            def f():
                for pauli, theta in terms:
                    qc.pauli_rotation(pauli, theta, reg)
            return f

        fs = [hadamard] + [batch(t) if kind == "batch" else loop(t) for _, kind, t, _ in cases] + [hadamard]
        for f in fs:
            f()                                                      # warm-up: code objects
        ts = [[] for _ in fs]
        for _ in range(reps):
            for k, f in enumerate(fs):
                reg.timer_start(); f(); ts[k].append(reg.timer_stop())
        had = ts[0] + ts[-1]
        lo, hi, med = min(had), max(had), statistics.median(had)
        gb = (32 << n) / 1e9                                         # one read and one write of the state
        rows.append({"case": f"hadamard_gate_{yard}", "n": n, "median_ms": round(med, 4), "spread_ms": [round(lo, 4), round(hi, 4)],
                     "series_medians_ms": [round(statistics.median(ts[0]), 4), round(statistics.median(ts[-1]), 4)],
                     "samples": len(had), "traffic_tb_per_s": round(gb / med, 3)})
        med_of = {}
        for (name, kind, terms, passes), t in zip(cases, ts[1:-1]):
            m = med_of[name, kind] = statistics.median(t)
            row = {"case": name, "kind": kind, "n": n, "terms": len(terms), "median_ms": round(m, 4), "min_ms": round(min(t), 4),
                   "max_ms": round(max(t), 4), "ratio_to_hadamard": round(m / med, 4)}
            if kind == "batch":
                tile = [0xFF | hot for _, hot in passes]
                p_of = qc.pauli_rotation_batch_plan(terms, n)[0]
                instr = sum((20 if x & tile[p] else 8) for ((x, _), _), p in zip(terms, p_of)) * (1 << n) / 64 / simds
                row.update({"passes": len(passes), "hot_masks": [hot for _, hot in passes], "ms_per_pass": round(m / len(passes), 4),
                            "traffic_tb_per_s": round(len(passes) * gb / m, 3), "fp64_wave_instructions_per_simd": round(instr),
                            "fp64_issue_fraction": round(instr * FP64_NS * 1e-6 / m, 3)})
            else:
                row.update({"passes": len(terms), "traffic_tb_per_s": round(len(terms) * gb / m, 3),
                            "batch_speedup": round(m / med_of[name, "batch"], 3),
                            "batch_is_not_slower": bool(med_of[name, "batch"] <= m)})
            rows.append(row)
    for r in rows:
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--simds", type=int, default=1024, help="SIMDs of the GPU (MI355X: 256 CUs of 4)")
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", help="JSON lines are appended here (default: profiles/pauli_rotation_batch_n<n>_timing.jsonl, started afresh)")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        step(a.n, a.reps, a.out, a.simds)
        return 0
    out = a.out
    if not out:
        out = os.path.join(ROOT, "profiles", f"pauli_rotation_batch_n{a.n}_timing.jsonl")
        open(out, "w").close()
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
           "--n", str(a.n), "--reps", str(a.reps), "--simds", str(a.simds), "--out", out, "--step"]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(json.dumps({"error": f"exit status {rc}"}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
