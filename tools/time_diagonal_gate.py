#!/usr/bin/env python3
"""Cost of qcx_diagonal_gate / qcx_diagonal_gate_device (K18, DESIGN s4.5n) on one GPU, dense fill_random state of n qubits.
The yardsticks are timed in the same process on the same register, never constants: hadamard_gate(12), one launch that reads
and writes every amplitude once (32 B per amplitude), and pauli_rotation with Z on every qubit (K15 SHAPE 0), the closest
kernel there was before: the same traffic plus a parity per amplitude.  The shapes (first, num):
  host form    (0,1) (0,8) (0,12) (5,7)   an entry per lane, the table inside a tile: timed twice, the lanes reading the table
                                          from memory (diag_lds = 0) and out of LDS (diag_lds = 1)
               (8,4) (12,4) (29,1) (10,10)  uniform entries: THE BAR -- no longer than 1.05 x the Z rotation
               (0,20)                     an entry per lane out of a 16-MiB table: the host maximum
  device form  (0,24) (0,n)               the table built by torch on the GPU; the call scans it first (one more read)
A host-form sample holds the table's copy to the device (16 B per entry) in front of the kernel.  And, once, what the call
replaces: a generic 12-qubit table as its 4095 Z strings through pauli_rotation_batch.
HIP events on the register's stream (timer_start / timer_stop) around each case.  The cases alternate, `--reps` rounds after a
warm-up call of each; the Hadamard is in every round TWICE, and the two series, identical work, give the run's own spread.
All rows are timed in ONE child process under `timeout`.  One JSON object per line, on stdout and in --out.

  python tools/time_diagonal_gate.py [--n 30] [--reps 9] [--out profiles/diagonal_gate_n30_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THETA = 0.37
BAR = 1.05


def shapes(n):
    host = [(0, 1), (0, 8), (0, 12), (5, 7), (8, 4), (12, 4), (n - 1, 1), (10, 10), (0, 20)]
    host = [(f, k) for f, k in host if f >= 0 and f + k <= n]
    dev = sorted({(0, min(24, n)), (0, n)})
    return host, dev


def step(n, reps, out, expansion):
    sys.path.insert(0, ROOT)
    import torch
    import quantumcomputer_amd as qc
    rs = np.random.RandomState(18)
    host, dev = shapes(n)
    rows = []
    with qc.Register(n, 0) as reg:
        reg.fill_random(30)
        reg.synchronize()
        yard = min(12, n - 1)
        tables = {s: qc.phase_table(rs.uniform(-np.pi, np.pi, 1 << s[1])) for s in host}
        dev_tables = {}
        for s in dev:
            ang = torch.rand(1 << s[1], dtype=torch.float64, device="cuda") * (2 * np.pi)
            dev_tables[s] = torch.polar(torch.ones_like(ang), ang)
            del ang
        torch.cuda.synchronize()
        torch.cuda.empty_cache()

        def hadamard():
            qc.hadamard_gate(yard, reg)

        def z_all():
            qc.pauli_rotation("Z" * n, THETA, reg)

        def host_call(s, lds):
            def f():
                qc.tune(diag_lds=lds)
                qc.diagonal_gate(s[0], s[1], tables[s], reg)
                qc.tune(diag_lds=0)
            return f

        def dev_call(s):
            return lambda: qc.diagonal_gate(s[0], s[1], dev_tables[s], reg)

        cases = [("host", s, 0) for s in host]
        cases += [("host", s, 1) for s in host if qc.diagonal_plan(n, *s)[1].form == qc.DIAG_LANE and s[0] + s[1] <= 12]
        cases += [("device", s, 0) for s in dev]
        fs = [hadamard, z_all] + [host_call(s, lds) if kind == "host" else dev_call(s) for kind, s, lds in cases] + [hadamard]
        for f in fs:
            f()                                                      # warm-up: code objects, the table scratch
        reg.synchronize()
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
        zmed = statistics.median(ts[1])
        rows.append({"case": "pauli_rotation_z_all", "n": n, "median_ms": round(zmed, 4), "min_ms": round(min(ts[1]), 4),
                     "max_ms": round(max(ts[1]), 4), "ratio_to_hadamard": round(zmed / med, 4), "traffic_tb_per_s": round(gb / zmed, 3)})
        for (kind, s, lds), t in zip(cases, ts[2:-1]):
            qc.tune(diag_lds=lds)
            pl = qc.diagonal_plan(n, *s)[1]
            qc.tune(diag_lds=0)
            m = statistics.median(t)
            table_bytes = 16 << s[1]
            row = {"case": f"diagonal_{s[0]}_{s[1]}", "n": n, "first": s[0], "num": s[1], "table": kind,
                   "form": ["tile", "group", "lane"][pl.form], "entry_source": "lds" if pl.lds else "memory", "kernel": pl.kernel.decode(),
                   "median_ms": round(m, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                   "ratio_to_z_rotation": round(m / zmed, 4), "ratio_to_hadamard": round(m / med, 4),
                   "state_bytes": 32 << n, "table_bytes": table_bytes, "slice_entries_per_tile": int(pl.slice_entries),
                   # what the sample moves besides the state: the host form's copy, the device form's scan; and the kernel's reads
                   "table_bytes_copied_or_scanned": table_bytes,
                   "table_bytes_read_by_lanes": (16 * int(pl.slice_entries)) << (n - 12) if not pl.lds else table_bytes * int(pl.grid)}
            if s[0] >= 8 and s[1] <= 12:
                row["bar"] = BAR
                row["meets_bar"] = bool(m <= BAR * zmed)
            rows.append(row)
        if expansion:
            # the same 12-qubit table as Z strings: every non-empty subset of qubits 0 .. 11 (angles: any, the cost is the passes')
            terms = [((0, z), float(rs.uniform(-1, 1))) for z in range(1, 1 << 12)]
            qc.pauli_rotation_batch(terms[:64], reg)                 # warm-up
            reg.timer_start(); qc.pauli_rotation_batch(terms, reg); t = reg.timer_stop()
            rows.append({"case": "z_string_expansion_of_12_qubits", "n": n, "terms": len(terms), "passes": reg.rotation_batch_stats()[0],
                         "ms": round(t, 2), "samples": 1})
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
    ap.add_argument("--no-expansion", action="store_true", help="skip the 4095-string pauli_rotation_batch (about 130 passes)")
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", help="JSON lines are appended here (default: profiles/diagonal_gate_n<n>_timing.jsonl, started afresh)")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        step(a.n, a.reps, a.out, not a.no_expansion)
        return 0
    out = a.out
    if not out:
        out = os.path.join(ROOT, "profiles", f"diagonal_gate_n{a.n}_timing.jsonl")
        open(out, "w").close()
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
           "--n", str(a.n), "--reps", str(a.reps), "--out", out, "--step"] + (["--no-expansion"] if a.no_expansion else [])
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(json.dumps({"error": f"exit status {rc}"}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
