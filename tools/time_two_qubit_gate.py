#!/usr/bin/env python3
"""Cost of qcx_two_qubit_gate / qcx_c_two_qubit_gate (K13, DESIGN s4.5g) on one GPU, dense fill_random state of n qubits.
The yardstick is always an existing kernel timed in the same process on the same register, never a constant.
  plain       per (q0, q1): two_qubit_ms (a seeded random 4x4 unitary) beside hadamard_lo_ms and hadamard_hi_ms, one
              qcx_hadamard_gate launch on the lower and on the higher of the two qubits.  All three move 32 * 2^n bytes;
              ratio = two_qubit_ms / max(hadamard_lo_ms, hadamard_hi_ms) (aim: <= 1.15).
  controlled  per (c, q0, q1): c_two_qubit_ms beside the two Hadamards and phase_ms, one qcx_c_phase_shift_gate(c, hi) launch.
              The gate moves the control-set half of the state (16 * 2^n bytes), twice the phase gate's bytes:
              ratio_per_byte = c_two_qubit_ms / (2 * phase_ms) (aim: <= 1.15 where all three qubits are >= 3; with a qubit
              below 3 the line forms run, and with the control below 3 they move the whole state).
HIP events on the register's stream (timer_start / timer_stop); the launches of a row alternate, the median of `--reps` each
after a warm-up call of each.  All rows are timed in ONE child process under `timeout`.  --tune KEY=VALUE sets a launch knob
(u2_variant, u2_nt, u2_streams_log2) for the run and is recorded in every row.  One JSON object per line, on stdout and
appended to --out.

  python tools/time_two_qubit_gate.py [--n 30] [--reps 9] [--out profiles/two_qubit_gate_n30_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAIN = [(0, 1), (1, 4), (2, 17), (3, 4), (5, 12), (12, 21), (21, 29), (28, 29)]
CONTROLLED = [(29, 3, 12), (5, 12, 21), (1, 5, 12), (12, 0, 21)]


def unitary(seed, d=4):
    import numpy as np
    rs = np.random.RandomState(seed)
    q, r = np.linalg.qr(rs.randn(d, d) + 1j * rs.randn(d, d))
    u = q * (np.diag(r) / np.abs(np.diag(r)))
    return np.clip(u.real, -1.0, 1.0) + 1j * np.clip(u.imag, -1.0, 1.0)


def form(n, c, lo):
    lowest = lo if c is None else min(c, lo)
    return "lines" if n >= 9 and lowest < 3 else "quad"


def step(n, reps, out, tune):
    sys.path.insert(0, ROOT)
    import math
    import quantumcomputer_amd as qc
    U = unitary(30)
    if tune:
        qc.tune(**tune)

    def medians(reg, *fs):
        """the launches alternate, so that all see the same neighbours and the same drift; median of `reps` each"""
        for f in fs:
            f()                                                      # warm-up: code objects, launch path
        ts = [[] for _ in fs]
        for _ in range(reps):
            for k, f in enumerate(fs):
                reg.timer_start(); f(); ts[k].append(reg.timer_stop())
        return [statistics.median(t) for t in ts]

    rows = []
    with qc.Register(n, 0) as reg:
        reg.fill_random(30)
        reg.synchronize()
        for q0, q1 in [(a, b) for a, b in PLAIN if a < n and b < n]:
            lo, hi = min(q0, q1), max(q0, q1)
            hl, hh, u = medians(reg, lambda: qc.hadamard_gate(lo, reg), lambda: qc.hadamard_gate(hi, reg), lambda: qc.two_qubit_gate(q0, q1, U, reg))
            rows.append({"kind": "plain", "n": n, "q0": q0, "q1": q1, "form": form(n, None, lo), "hadamard_lo_ms": round(hl, 4),
                         "hadamard_hi_ms": round(hh, 4), "two_qubit_ms": round(u, 4), "ratio": round(u / max(hl, hh), 4),
                         "two_qubit_tb_per_s": round((32 << n) / 1e9 / u, 3)})
        for c, q0, q1 in [(c, a, b) for c, a, b in CONTROLLED if max(c, a, b) < n]:
            lo, hi = min(q0, q1), max(q0, q1)
            theta = math.pi / 8
            hl, hh, p, u = medians(reg, lambda: qc.hadamard_gate(lo, reg), lambda: qc.hadamard_gate(hi, reg),
                                   lambda: qc.c_phase_shift_gate(c, hi, theta, reg), lambda: qc.c_two_qubit_gate(c, q0, q1, U, reg))
            rows.append({"kind": "controlled", "n": n, "c": c, "q0": q0, "q1": q1, "form": form(n, c, lo), "hadamard_lo_ms": round(hl, 4),
                         "hadamard_hi_ms": round(hh, 4), "phase_ms": round(p, 4), "c_two_qubit_ms": round(u, 4),
                         "ratio_per_byte": round(u / (2 * p), 4), "c_two_qubit_tb_per_s": round((16 << n) / 1e9 / u, 3)})
    for r in rows:
        if tune:
            r["tune"] = tune
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE", help="a launch knob for this run (recorded in every row)")
    ap.add_argument("--out", help="JSON lines are appended here (default: profiles/two_qubit_gate_n<n>_timing.jsonl, started afresh)")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    tune = {k: int(v) for k, v in (kv.split("=", 1) for kv in a.tune)}
    if a.step:
        step(a.n, a.reps, a.out, tune)
        return 0
    out = a.out
    if not out:
        out = os.path.join(ROOT, "profiles", f"two_qubit_gate_n{a.n}_timing.jsonl")
        open(out, "w").close()
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
           "--n", str(a.n), "--reps", str(a.reps), "--out", out, "--step"] + [x for kv in a.tune for x in ("--tune", kv)]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(json.dumps({"error": f"exit status {rc}"}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
