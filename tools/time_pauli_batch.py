#!/usr/bin/env python3
"""Cost of qcx_pauli_expectation_batch (K14b, DESIGN s4.5h) on one GPU, dense fill_random state of n qubits: groups of K terms
that share an x_mask, K = 1, 2, 8 and W = qcx_pauli_batch_width(), in the shapes of the first stage
  z        x_mask = 0                            (a tile, no partner)
  x_q5     X or Y on qubit 5                     (a tile, the partner inside it: one LDS exchange)
  x_top    X or Y on the highest qubit           (pairs of tiles)
  xyz_all  X or Y on two qubits of every three   (pairs of tiles, partner offsets of every kind)
with K distinct random z_masks each (so Y's and both parities of g occur), and a Heisenberg chain: XX + YY + ZZ on every
bond (q, q + 1).  The yardsticks are timed in the same process on the same register, never constants: expectation_sum on the
SAME terms (one read per term), and marginal(0, 0) (the same bytes through one tree).  The batch call is never timed against
itself.  HIP events on the register's stream (timer_start / timer_stop) around each call; the launches alternate, `--reps`
rounds after a warm-up call of each, medians.  marginal(0, 0) is in every round TWICE: the two series, identical work, give
the run's own spread.  A row's extra_term_ms is (batch(K) - batch(1)) / (K - 1) within its shape.  All rows are timed in ONE
child process under `timeout`.  One JSON object per line, on stdout and in --out.

  python tools/time_pauli_batch.py [--n 30] [--reps 9] [--out profiles/pauli_batch_n30_timing.jsonl]
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shapes(n):
    xyz = sum(1 << q for q in range(n) if q % 3 != 2)
    return [("z", 0), ("x_q5", 1 << min(5, n - 1)), ("x_top", 1 << (n - 1)), ("xyz_all", xyz)]


def group(n, x, k, seed):
    rs = random.Random(seed)
    zs = set()
    while len(zs) < k:
        zs.add(rs.getrandbits(n))
    return [(1.0, (x, z)) for z in sorted(zs)]


def heisenberg(n):
    terms = []
    for q in range(n - 1):
        for p in "XYZ":
            terms.append((1.0, {q: p, q + 1: p}))
    return terms


def step(n, reps, out):
    sys.path.insert(0, ROOT)
    import quantumcomputer_amd as qc
    W = qc.pauli_batch_width()
    cases = [(name, k, group(n, x, k, 100 * k + i)) for i, (name, x) in enumerate(shapes(n)) for k in (1, 2, 8, W)]
    cases.append(("heisenberg_chain", 0, heisenberg(n)))
    rows = []
    with qc.Register(n, 0) as reg:
        reg.fill_random(30)
        reg.synchronize()
        fs = [lambda: reg.marginal(0, 0)]
        for _, _, terms in cases:
            fs.append((lambda t: lambda: reg.expectation_batch(t))(terms))
            fs.append((lambda t: lambda: reg.expectation_sum(t))(terms))
        fs.append(lambda: reg.marginal(0, 0))
        same = True
        for i, f in enumerate(fs):                                   # warm-up: code objects, the stages' buffer
            r = f()
            if 0 < i < len(fs) - 1 and i % 2 == 0:                   # ... and the two calls agree bit for bit
                same = same and r[1].tobytes() == last[1].tobytes() and r[0] == last[0]
            last = r
        ts = [[] for _ in fs]
        for _ in range(reps):
            for k, f in enumerate(fs):
                reg.timer_start(); f(); ts[k].append(reg.timer_stop())
        marg = ts[0] + ts[-1]
        lo, hi, med = min(marg), max(marg), statistics.median(marg)
        rows.append({"case": "marginal_0_0", "n": n, "median_ms": round(med, 4), "spread_ms": [round(lo, 4), round(hi, 4)],
                     "series_medians_ms": [round(statistics.median(ts[0]), 4), round(statistics.median(ts[-1]), 4)],
                     "samples": len(marg), "batch_width": W, "batch_equals_sum_bitwise": bool(same)})
        first = {}
        for i, (name, k, terms) in enumerate(cases):
            tb, tsum = ts[1 + 2 * i], ts[2 + 2 * i]
            mb, ms = statistics.median(tb), statistics.median(tsum)
            xs = [qc.pauli_masks(p, n)[0] for _, p in terms]
            row = {"case": name, "n": n, "terms": len(terms), "distinct_x_masks": len(set(xs)), "passes": qc.pauli_batch_plan(xs)[1],
                   "batch_median_ms": round(mb, 4), "batch_min_ms": round(min(tb), 4), "batch_max_ms": round(max(tb), 4),
                   "sum_median_ms": round(ms, 4), "sum_min_ms": round(min(tsum), 4), "sum_max_ms": round(max(tsum), 4),
                   "batch_over_sum": round(mb / ms, 4), "batch_over_marginal": round(mb / med, 4)}
            if k:
                row["x_mask"] = xs[0]
                row["shape"] = "pair" if xs[0] >> 12 else ("tile, exchange" if xs[0] else "tile")
                first.setdefault(name, mb)
                if k > 1:
                    row["extra_term_ms"] = round((mb - first[name]) / (k - 1), 4)
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
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", help="JSON lines are appended here (default: profiles/pauli_batch_n<n>_timing.jsonl, started afresh)")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        step(a.n, a.reps, a.out)
        return 0
    out = a.out
    if not out:
        out = os.path.join(ROOT, "profiles", f"pauli_batch_n{a.n}_timing.jsonl")
        open(out, "w").close()
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
           "--n", str(a.n), "--reps", str(a.reps), "--out", out, "--step"]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(json.dumps({"error": f"exit status {rc}"}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
