#!/usr/bin/env python3
"""Cost of qcx_reduced_density_matrix (K16, DESIGN s4.5j) on one GPU, dense fill_random state of n qubits: ranges of num = 1, 2
and 4 qubits at first = 0 (the range inside a thread's lines), first = 10 (num = 4 straddles unit bit 12) and first = n - num
(the range above the unit).  The yardsticks are timed in the same process on the same register, never constants:
marginal(0, 0) (the same bytes through one tree), and the tomography route the call replaces -- all 4^num Pauli strings on the
range through expectation_batch, which serves the strings that share an x_mask in one read: 2^num reads of the state.
HIP events on the register's stream (timer_start / timer_stop) around each call; the launches alternate, `--reps` rounds after
a warm-up call of each, the best and the median of a series are reported.  Every row also says whether the call read the state
once (rdm_stats) and how far the matrix rebuilt from the tomography values is from it.  All rows are timed in ONE child
process under `timeout`.  One JSON object per line, on stdout and in --out.

  python tools/time_rdm.py [--n 30] [--reps 5] [--out profiles/rdm_n30_timing.jsonl]
"""
import argparse
import itertools
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAULI = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}


def tomography_terms(first, num):
    return [(1.0, {first + k: p for k, p in enumerate(s)}) for s in itertools.product("IXYZ", repeat=num)]


def from_tomography(num, values):
    """rho = 2^-num sum_P <P> P, qubit first + k = bit k of the matrix index"""
    rho = np.zeros((1 << num, 1 << num), dtype=np.complex128)
    for s, v in zip(itertools.product("IXYZ", repeat=num), values):
        P = np.eye(1)
        for p in s:
            P = np.kron(PAULI[p], P)
        rho += v * P
    return rho / (1 << num)


def step(n, reps, out):
    sys.path.insert(0, ROOT)
    import quantumcomputer_amd as qc
    cases = []
    for num in (1, 2, 4):
        for first in sorted({0, min(10, n - num), n - num}):
            cases.append((first, num, tomography_terms(first, num)))
    rows = []
    with qc.Register(n, 0) as reg:
        reg.fill_random(30)
        reg.synchronize()
        fs = [lambda: reg.marginal(0, 0)]
        for first, num, terms in cases:
            fs.append((lambda f, k: lambda: reg.reduced_density_matrix(f, k))(first, num))
            fs.append((lambda t: lambda: reg.expectation_batch(t))(terms))
        fs.append(lambda: reg.marginal(0, 0))
        checks = []
        for i, f in enumerate(fs):                                   # warm-up: code objects, the stages' buffer
            r = f()
            if 0 < i < len(fs) - 1 and i % 2 == 1:
                rho, stats = r, reg.rdm_stats()
            elif 0 < i < len(fs) - 1:
                num = cases[(i - 1) // 2][1]
                checks.append((stats, float(np.max(np.abs(from_tomography(num, r[1]) - rho))), reg.expectation_stats()[1]))
        ts = [[] for _ in fs]
        for _ in range(reps):
            for k, f in enumerate(fs):
                reg.timer_start(); f(); ts[k].append(reg.timer_stop())
        marg = ts[0] + ts[-1]
        med = statistics.median(marg)
        rows.append({"case": "marginal_0_0", "n": n, "best_ms": round(min(marg), 4), "median_ms": round(med, 4),
                     "spread_ms": [round(min(marg), 4), round(max(marg), 4)], "samples": len(marg)})
        for i, (first, num, terms) in enumerate(cases):
            tr, tt = ts[1 + 2 * i], ts[2 + 2 * i]
            stats, dist, reads = checks[i]
            rows.append({"case": "rdm", "n": n, "first": first, "num": num, "source": stats[0], "state_reads": stats[1],
                         "best_ms": round(min(tr), 4), "median_ms": round(statistics.median(tr), 4), "max_ms": round(max(tr), 4),
                         "tomography_strings": len(terms), "tomography_reads": reads,
                         "tomography_best_ms": round(min(tt), 4), "tomography_median_ms": round(statistics.median(tt), 4),
                         "over_marginal": round(min(tr) / min(marg), 4), "over_tomography": round(min(tr) / min(tt), 4),
                         "max_abs_difference_from_tomography": dist})
    for r in rows:
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", help="JSON lines are appended here (default: profiles/rdm_n<n>_timing.jsonl, started afresh)")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        step(a.n, a.reps, a.out)
        return 0
    out = a.out
    if not out:
        out = os.path.join(ROOT, "profiles", f"rdm_n{a.n}_timing.jsonl")
        open(out, "w").close()
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
           "--n", str(a.n), "--reps", str(a.reps), "--out", out, "--step"]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(json.dumps({"error": f"exit status {rc}"}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
