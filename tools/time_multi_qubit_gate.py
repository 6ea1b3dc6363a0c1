#!/usr/bin/env python3
"""Cost of qcx_mc_multi_qubit_gate (K20, DESIGN s4.5p) on one GPU, dense fill_random state of n qubits.
The yardsticks are timed in the same process on the same register, never constants:
  (a) hadamard_gate(12)                  one launch that reads and writes every amplitude once (32 B per amplitude)
  (b) permutation_gate(first, k)         on the same contiguous range: K19's tile is K20's, the same loads and stores with no
                                         arithmetic, so the difference is the cost of the products (contiguous shapes only: no
                                         range gives a spread target set's tile)
  (c) gate_batch(QFT on the k targets)   the fastest way to the same operator there was: H and controlled phases as a list;
                                         the new call takes fused_matrix of that very list
The new call, a random unitary on
  k = 3, 4, 5 contiguous low (3 ..), contiguous high (25 ..), inside a line (0, 1, 2), spread (3, 14, 22, 29) and
  (2, 9, 14, 22, 29); (3, 4, 5, 6) under one, two and three controls at bits >= 3 (squeezed: traffic 2^-k) and under one control
  at bit 0 (a predicate), the latter also with multi_store_all = 0.
HIP events on the register's stream (timer_start / timer_stop) around each case.  The cases alternate, `--reps` rounds after a
warm-up call of each; the Hadamard is in every round TWICE, and the two series, identical work, give the run's own spread.
All rows are timed in ONE child process under `timeout`.  One JSON object per line, on stdout and in --out.

  python tools/time_multi_qubit_gate.py [--n 30] [--reps 9] [--out profiles/multi_qubit_gate_n30_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"multi_nt": 0, "multi_store_all": 1}


def random_unitary(seed, d):
    rs = np.random.RandomState(seed)
    q, r = np.linalg.qr(rs.randn(d, d) + 1j * rs.randn(d, d))
    u = q * (np.diag(r) / np.abs(np.diag(r)))
    return np.clip(u.real, -1.0, 1.0) + 1j * np.clip(u.imag, -1.0, 1.0)


def qft_gates(qubits):
    """the QFT on `qubits` (first = most significant) as H and controlled phases, in gate_batch's form; no final swaps"""
    H = np.array([[1, 1], [1, -1]], dtype=complex) / np.sqrt(2.0)
    gates = []
    for i, q in enumerate(qubits):
        gates.append((H, q))
        for j, c in enumerate(qubits[i + 1:], start=2):
            gates.append((np.diag([1.0, np.exp(2j * np.pi / (1 << j))]), q, c))
    return gates


def step(n, reps, out):
    sys.path.insert(0, ROOT)
    import quantumcomputer_amd as qc
    rows = []
    with qc.Register(n, 0) as reg:
        reg.fill_random(30)
        reg.synchronize()
        yard = min(12, n - 1)
        hi = n - 5
        shapes = [(3, 4, 5), (hi, hi + 1, hi + 2), (0, 1, 2), (3, 4, 5, 6), (hi, hi + 1, hi + 2, hi + 3), (3, 14, 22, n - 1),
                  (3, 4, 5, 6, 7), (hi, hi + 1, hi + 2, hi + 3, hi + 4), (2, 9, 14, 22, n - 1)]
        shapes = [t for t in shapes if len(set(t)) == len(t) and max(t) < n and sorted(t) == list(t)]

        def hadamard():
            qc.hadamard_gate(yard, reg)

        def multi_call(targets, U, controls, knobs):
            cm = sum(1 << c for c in controls)
            cv = sum(1 << c for c, v in controls.items() if v)

            def f():
                if knobs:
                    qc.tune(**knobs)
                qc.multi_qubit_gate(targets, U, reg, controls=cm, values=cv)
                if knobs:
                    qc.tune(**{k: DEFAULTS[k] for k in knobs})
            return f

        def perm_call(first, k, table):
            return lambda: qc.permutation_gate(first, k, table, reg)

        def batch_call(gates):
            return lambda: qc.gate_batch(gates, reg)

        # (label, kind, targets, controls, knobs, callable)
        cases = []
        rs = np.random.RandomState(19)
        for t in shapes:
            k = len(t)
            name = "_".join(str(q) for q in t)
            cases.append((f"multi_{name}", "multi", t, {}, {}, multi_call(t, random_unitary(k, 1 << k), {}, {})))
            if t == tuple(range(t[0], t[0] + k)):
                cases.append((f"permutation_{t[0]}_{k}", "permutation", t, {}, {}, perm_call(t[0], k, rs.permutation(1 << k))))
            gates = qft_gates(list(t)[::-1])
            F = qc.fused_matrix(gates, t)
            F = np.clip(F.real, -1, 1) + 1j * np.clip(F.imag, -1, 1)
            cases.append((f"qft_fused_{name}", "multi", t, {}, {}, multi_call(t, F, {}, {})))
            cases.append((f"qft_gate_batch_{name}", "gate_batch", t, {}, {"gates": len(gates)}, batch_call(gates)))
        t4 = (3, 4, 5, 6)
        if n >= 24:
            U4 = random_unitary(44, 16)
            for label, controls, knobs in [("c20", {20: 1}, {}), ("c20_c21", {20: 1, 21: 0}, {}), ("c20_c21_c22", {20: 1, 21: 0, 22: 1}, {}),
                                           ("c12_c13_c14", {12: 1, 13: 1, 14: 1}, {}), ("c0", {0: 1}, {}), ("c0_no_store_all", {0: 1}, {"multi_store_all": 0})]:
                cases.append((f"controlled_3_4_5_6_{label}", "multi", t4, controls, knobs, multi_call(t4, U4, controls, knobs)))
        fs = [hadamard] + [c[5] for c in cases] + [hadamard]
        for f in fs:
            f()                                                      # warm-up: code objects, the matrix scratch
        reg.synchronize()
        ts = [[] for _ in fs]
        for _ in range(reps):
            for k, f in enumerate(fs):
                reg.timer_start(); f(); ts[k].append(reg.timer_stop())
        had = ts[0] + ts[-1]
        lo, hi_, med = min(had), max(had), statistics.median(had)
        gb = (32 << n) / 1e9                                         # one read and one write of the state
        rows.append({"case": f"hadamard_gate_{yard}", "n": n, "median_ms": round(med, 4), "spread_ms": [round(lo, 4), round(hi_, 4)],
                     "series_medians_ms": [round(statistics.median(ts[0]), 4), round(statistics.median(ts[-1]), 4)],
                     "samples": len(had), "traffic_tb_per_s": round(gb / med, 3)})
        for (label, kind, t, controls, knobs, _), samples in zip(cases, ts[1:-1]):
            m = statistics.median(samples)
            row = {"case": label, "kind": kind, "n": n, "targets": list(t), "controls": {str(c): v for c, v in controls.items()}, "knobs": knobs,
                   "median_ms": round(m, 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4), "ratio_to_hadamard": round(m / med, 4)}
            if kind == "multi":
                cm = sum(1 << c for c in controls)
                cv = sum(1 << c for c, v in controls.items() if v)
                pl = qc.multi_gate_plan(n, cm, cv, t)[1]
                fires = (1 << n) >> sum(1 for c in controls if c >= 3)
                row.update({"kernel": pl.kernel.decode(), "T": pl.T, "units": int(pl.units), "grid": pl.grid, "block": pl.block, "lds_bytes": pl.lds_bytes,
                            "store_all": pl.store_all, "bytes_moved": 32 * fires, "tb_per_s": round(32 * fires / 1e9 / m, 3),
                            "fp64_ops": 8 * (1 << len(t)) * ((1 << n) >> len(controls)), "fp64_tops": round(8 * (1 << len(t)) * ((1 << n) >> len(controls)) / 1e9 / m, 3)})
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
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", help="JSON lines are appended here (default: profiles/multi_qubit_gate_n<n>_timing.jsonl, started afresh)")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        step(a.n, a.reps, a.out)
        return 0
    out = a.out
    if not out:
        out = os.path.join(ROOT, "profiles", f"multi_qubit_gate_n{a.n}_timing.jsonl")
        open(out, "w").close()
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
           "--n", str(a.n), "--reps", str(a.reps), "--out", out, "--step"]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(json.dumps({"error": f"exit status {rc}"}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
