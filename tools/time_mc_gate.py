#!/usr/bin/env python3
"""Cost of qcx_mc_one_qubit_gate / qcx_mc_two_qubit_gate (K17, DESIGN s4.5m) on one GPU, dense fill_random state of n qubits.
The yardstick is always an existing call timed in the same process on the same register, never a constant.  One sample (one run
of this tool) is a set of rows:
  toffoli     per (c0, c1, t) -- controls high (n-2, n-1), mid (10, 20) and low (0, 1), t = 15: mc_ms, the Toffoli as
              mc_one_qubit_gate({c0, c1}, t, X), beside c_two_qubit_ms, the same gate as c_two_qubit_gate(c0, c1, t, CNOT), the
              only way before K17.  not_slower = mc_ms <= c_two_qubit_ms + the spread (max - min) of that yardstick's own samples.
  controls    k = 1, 3, 5, 10 and n - 1 positive controls (the highest qubits) on target 12: mc_ms and the bytes the form moves
  negative    one negative control (n - 1) beside the positive one, target 12
  ccswap      SWAP on (5, 15) under (n-2, n-1)
  same_launch one positive control through the new call (mc_generic = 0: c_one_qubit_gate's launch) beside c_one_qubit_gate
  yardsticks  hadamard_gate(12) and c_one_qubit_gate(n - 1, 12)
bytes = what the form reads and writes: 32 * count pairs (64 * count quads; 32 * count amplitudes in the shuffle forms); tb_per_s
from them.  HIP events on the register's stream (timer_start / timer_stop); the launches of a row alternate, the median of
`--reps` each after a warm-up call of each.  All rows are timed in ONE child process under `timeout`.  --tune KEY=VALUE sets a
launch knob for the run and is recorded in every row.  One JSON object per line, on stdout and appended to --out.

  python tools/time_mc_gate.py [--n 30] [--reps 9] [--out profiles/mc_gate_n30_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_row(qc, n, mask, vals, targets):
    st, pl = qc.mc_gate_plan(n, mask, vals, targets)
    assert st == 0
    per_item = {qc._lib.MC_PAIR: 32, qc._lib.MC_LINE_PAIR: 32, qc._lib.MC_LINE_SHFL: 16, qc._lib.MC_QUAD: 64}.get(pl.form, 64 >> pl.ns)
    return {"kernel": pl.kernel.decode(), "count": int(pl.count), "bytes": 2 * per_item * int(pl.count)}


def step(n, reps, out, tune):
    sys.path.insert(0, ROOT)
    import quantumcomputer_amd as qc
    if tune:
        qc.tune(**tune)
    X, CNOT, SWAP = qc.GATES["X"], qc.GATES2["CNOT"], qc.GATES2["SWAP"]
    T, S = n - 1, n - 2

    def samples(reg, *fs):
        """the launches alternate, so that all see the same neighbours and the same drift; `reps` samples each"""
        for f in fs:
            f()                                                      # warm-up: code objects, launch path
        ts = [[] for _ in fs]
        for _ in range(reps):
            for k, f in enumerate(fs):
                reg.timer_start(); f(); ts[k].append(reg.timer_stop())
        return ts

    med = statistics.median
    rows = []
    with qc.Register(n, 0) as reg:
        reg.fill_random(30)
        reg.synchronize()
        h, cu, mc1 = samples(reg, lambda: qc.hadamard_gate(12, reg), lambda: qc.c_one_qubit_gate(T, 12, X, reg),
                             lambda: qc.mc_one_qubit_gate([T], 12, X, reg))
        rows.append({"kind": "yardsticks", "n": n, "hadamard_12_ms": round(med(h), 4), "c_one_qubit_ms": round(med(cu), 4),
                     "c_one_qubit_spread_ms": round(max(cu) - min(cu), 4)})
        rows.append({"kind": "same_launch", "n": n, "controls": [T], "target": 12, "mc_ms": round(med(mc1), 4), "c_one_qubit_ms": round(med(cu), 4),
                     "same_cost": bool(abs(med(mc1) - med(cu)) <= max(cu) - min(cu) + max(mc1) - min(mc1))})
        for where, (c0, c1) in (("high", (S, T)), ("mid", (10, 20)), ("low", (0, 1))):
            t = 15
            old, new = samples(reg, lambda: qc.c_two_qubit_gate(c0, c1, t, CNOT, reg), lambda: qc.mc_one_qubit_gate([c0, c1], t, X, reg))
            r = {"kind": "toffoli", "n": n, "controls": [c0, c1], "where": where, "target": t, "mc_ms": round(med(new), 4),
                 "c_two_qubit_ms": round(med(old), 4), "c_two_qubit_spread_ms": round(max(old) - min(old), 4),
                 "not_slower": bool(med(new) <= med(old) + (max(old) - min(old)))}
            r.update(plan_row(qc, n, (1 << c0) | (1 << c1), (1 << c0) | (1 << c1), (t,)))
            r["tb_per_s"] = round(r["bytes"] / 1e9 / med(new), 3)
            rows.append(r)
        for k in (1, 3, 5, 10, n - 1):
            cs = [q for q in range(n - 1, -1, -1) if q != 12][:k]
            mask = sum(1 << c for c in cs)
            (new,) = samples(reg, lambda: qc.mc_one_qubit_gate(mask, 12, X, reg))
            r = {"kind": "controls", "n": n, "k": k, "target": 12, "mc_ms": round(med(new), 4)}
            if k > 1:                                                 # (k = 1 is c_one_qubit_gate's launch unless mc_generic is set)
                r.update(plan_row(qc, n, mask, mask, (12,)))
                r["tb_per_s"] = round(r["bytes"] / 1e9 / med(new), 3)
            rows.append(r)
        pos, neg = samples(reg, lambda: qc.mc_one_qubit_gate([T], 12, X, reg), lambda: qc.mc_one_qubit_gate([T], 12, X, reg, values=0))
        r = {"kind": "negative", "n": n, "control": T, "target": 12, "positive_ms": round(med(pos), 4), "negative_ms": round(med(neg), 4)}
        r.update(plan_row(qc, n, 1 << T, 0, (12,)))
        rows.append(r)
        (sw,) = samples(reg, lambda: qc.mc_two_qubit_gate([S, T], 5, 15, SWAP, reg))
        r = {"kind": "ccswap", "n": n, "controls": [S, T], "targets": [5, 15], "mc_ms": round(med(sw), 4)}
        r.update(plan_row(qc, n, (1 << S) | (1 << T), (1 << S) | (1 << T), (5, 15)))
        r["tb_per_s"] = round(r["bytes"] / 1e9 / med(sw), 3)
        rows.append(r)
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
    ap.add_argument("--out", help="JSON lines are appended here (default: profiles/mc_gate_n<n>_timing.jsonl)")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    tune = {k: int(v) for k, v in (kv.split("=", 1) for kv in a.tune)}
    if a.step:
        step(a.n, a.reps, a.out, tune)
        return 0
    out = a.out or os.path.join(ROOT, "profiles", f"mc_gate_n{a.n}_timing.jsonl")
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
           "--n", str(a.n), "--reps", str(a.reps), "--out", out, "--step"] + [x for kv in a.tune for x in ("--tune", kv)]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(json.dumps({"error": f"exit status {rc}"}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
