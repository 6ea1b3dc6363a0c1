#!/usr/bin/env python3
"""Cost of qcx_pauli_rotation (K15, DESIGN s4.5i) on one GPU, dense fill_random state of n qubits.
The yardstick is hadamard_gate(12) timed in the same process on the same register, never a constant: one launch that reads and
writes every amplitude once (32 B per amplitude), which is all a rotation moves, for any string.  The strings:
  z_all     Z on every qubit                     (a tile, no partner: a streaming diagonal)
  x_q5      X on qubit 5                         (a tile, the partner inside it: one LDS exchange)
  x_top     X on the highest qubit               (pairs of tiles)
  xyz_all   X, Y, Z, X, Y, Z, ... on all qubits  (pairs of tiles, partner offsets and signs of every kind)
  eight     X Y Z X Y Z X Y on eight qubits spread evenly from qubit 0 to the highest (both sides of tile bit 12)
and `eight_decomposed`: the same unitary as `eight` the textbook way, from one_qubit_gate / two_qubit_gate calls -- a basis
change on every X / Y qubit, a CNOT ladder, one rz, the ladder and the basis changes undone: 2 * 6 + 2 * 7 + 1 = 27 passes.
HIP events on the register's stream (timer_start / timer_stop) around each case.  The cases alternate, `--reps` rounds after a
warm-up call of each; the Hadamard is in every round TWICE, and the two series, identical work, give the run's own spread:
spread_ms = [the least, the greatest] of all Hadamard samples.  All rows are timed in ONE child process under `timeout`.  One
JSON object per line, on stdout and in --out.

  python tools/time_pauli_rotation.py [--n 30] [--reps 9] [--out profiles/pauli_rotation_n30_timing.jsonl]
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


def eight(n):
    qs = sorted({round(k * (n - 1) / 7) for k in range(8)})
    return {q: "XYZXYZXY"[k] for k, q in enumerate(qs)}


def strings(n):
    return [("z_all", "Z" * n), ("x_q5", {min(5, n - 1): "X"}), ("x_top", {n - 1: "X"}), ("xyz_all", ("XYZ" * n)[:n]), ("eight", eight(n))]


def decomposition(pauli, theta, gates, gates2, rz):
    """exp(-i theta/2 P) for the dict `pauli` as a list of ("u1", q, U) / ("u2", q0, q1, U) calls, in the order they are applied:
    X = H Z H and Y = (S H) Z (S H)^+ turn every letter into Z, a CNOT ladder gathers the parity of those qubits in the last one,
    rz(theta) acts there, and everything is undone"""
    H, S = np.asarray(gates["H"]), np.asarray(gates["S"])
    qs = sorted(q for q, p in pauli.items() if p != "I")
    pre = [("u1", q, H if pauli[q] == "X" else H @ S.conj().T) for q in qs if pauli[q] in "XY"]
    post = [("u1", q, H if pauli[q] == "X" else S @ H) for q in qs if pauli[q] in "XY"]
    ladder = [("u2", a, b, np.asarray(gates2["CNOT"])) for a, b in zip(qs, qs[1:])]
    return pre + ladder + [("u1", qs[-1], rz(theta))] + ladder[::-1] + post


def step(n, reps, out):
    sys.path.insert(0, ROOT)
    import quantumcomputer_amd as qc
    cases = strings(n)
    ops = decomposition(eight(n), THETA, qc.GATES, qc.GATES2, qc.rz)
    rows = []
    with qc.Register(n, 0) as reg:
        reg.fill_random(30)
        reg.synchronize()
        yard = min(12, n - 1)

        def decomposed():
            for op in ops:
                if op[0] == "u1":
                    qc.one_qubit_gate(op[1], op[2], reg)
                else:
                    qc.two_qubit_gate(op[1], op[2], op[3], reg)

        def hadamard():
            qc.hadamard_gate(yard, reg)

        fs = [hadamard] + [(lambda p: lambda: qc.pauli_rotation(p, THETA, reg))(p) for _, p in cases] + [decomposed, hadamard]
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
        for (name, p), t in zip(cases, ts[1:-2]):
            x, z = qc.pauli_masks(p, n)
            m = med_of[name] = statistics.median(t)
            rows.append({"case": name, "n": n, "x_mask": x, "z_mask": z,
                         "shape": "pair" if x >> 12 else ("tile, exchange" if x else "tile"),
                         "median_ms": round(m, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                         "ratio_to_hadamard": round(m / med, 4), "inside_hadamard_spread": bool(lo <= m <= hi),
                         "traffic_tb_per_s": round(gb / m, 3)})
        t = ts[-2]
        m = statistics.median(t)
        rows.append({"case": "eight_decomposed", "n": n, "passes": len(ops), "median_ms": round(m, 4), "min_ms": round(min(t), 4),
                     "max_ms": round(max(t), 4), "ratio_to_hadamard": round(m / med, 4),
                     "ratio_to_the_rotation": round(m / med_of["eight"], 4)})
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
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", help="JSON lines are appended here (default: profiles/pauli_rotation_n<n>_timing.jsonl, started afresh)")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        step(a.n, a.reps, a.out)
        return 0
    out = a.out
    if not out:
        out = os.path.join(ROOT, "profiles", f"pauli_rotation_n{a.n}_timing.jsonl")
        open(out, "w").close()
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
           "--n", str(a.n), "--reps", str(a.reps), "--out", out, "--step"]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(json.dumps({"error": f"exit status {rc}"}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
