#!/usr/bin/env python3
"""Cost of qcx_pauli_expectation (K14, DESIGN s4.5h) on one GPU, dense fill_random state of n qubits.
The yardstick is marginal(0, 0) timed in the same process on the same register, never a constant: it moves the same bytes
through the same tree, only its leaf is |a|^2.  The strings:
  z_all     Z on every qubit                     (a tile, no partner: the marginal's own shape with a sign)
  x_q5      X on qubit 5                         (a tile, the partner inside it: one LDS exchange)
  x_top     X on the highest qubit               (pairs of tiles)
  xyz_all   X, Y, Z, X, Y, Z, ... on all qubits  (pairs of tiles, partner offsets and signs of every kind)
HIP events on the register's stream (timer_start / timer_stop) around each call: the stages and the copy of the one double.
The launches alternate, `--reps` rounds after a warm-up call of each; marginal(0, 0) is in every round TWICE, and the two
series, identical work, give the run's own spread: spread_ms = [the least, the greatest] of all marginal samples.  A string's
row says whether its median lies inside it.  All rows are timed in ONE child process under `timeout`.  One JSON object per
line, on stdout and in --out.

  python tools/time_pauli_expectation.py [--n 30] [--reps 9] [--out profiles/pauli_expectation_n30_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def strings(n):
    return [("z_all", "Z" * n), ("x_q5", {min(5, n - 1): "X"}), ("x_top", {n - 1: "X"}), ("xyz_all", ("XYZ" * n)[:n])]


def step(n, reps, out):
    sys.path.insert(0, ROOT)
    import quantumcomputer_amd as qc
    cases = strings(n)
    rows = []
    with qc.Register(n, 0) as reg:
        reg.fill_random(30)
        reg.synchronize()
        fs = [lambda: reg.marginal(0, 0)] + [(lambda p: lambda: reg.expectation(p))(p) for _, p in cases] + [lambda: reg.marginal(0, 0)]
        for f in fs:
            f()                                                      # warm-up: code objects, the stages' buffer
        ts = [[] for _ in fs]
        for _ in range(reps):
            for k, f in enumerate(fs):
                reg.timer_start(); f(); ts[k].append(reg.timer_stop())
        marg = ts[0] + ts[-1]
        lo, hi, med = min(marg), max(marg), statistics.median(marg)
        gb = (16 << n) / 1e9
        rows.append({"case": "marginal_0_0", "n": n, "median_ms": round(med, 4), "spread_ms": [round(lo, 4), round(hi, 4)],
                     "series_medians_ms": [round(statistics.median(ts[0]), 4), round(statistics.median(ts[-1]), 4)],
                     "samples": len(marg), "state_tb_per_s": round(gb / med, 3)})
        for (name, p), t in zip(cases, ts[1:-1]):
            x, z = qc.pauli_masks(p, n)
            m = statistics.median(t)
            rows.append({"case": name, "n": n, "x_mask": x, "z_mask": z,
                         "shape": "pair" if x >> 12 else ("tile, exchange" if x else "tile"),
                         "median_ms": round(m, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                         "ratio_to_marginal": round(m / med, 4), "inside_marginal_spread": bool(lo <= m <= hi),
                         "state_tb_per_s": round(gb / m, 3)})
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
    ap.add_argument("--out", help="JSON lines are appended here (default: profiles/pauli_expectation_n<n>_timing.jsonl, started afresh)")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        step(a.n, a.reps, a.out)
        return 0
    out = a.out
    if not out:
        out = os.path.join(ROOT, "profiles", f"pauli_expectation_n{a.n}_timing.jsonl")
        open(out, "w").close()
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
           "--n", str(a.n), "--reps", str(a.reps), "--out", out, "--step"]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(json.dumps({"error": f"exit status {rc}"}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
