#!/usr/bin/env python3
"""Cost of qcx_permutation_gate (K19, DESIGN s4.5o) on one GPU, dense fill_random state of n qubits on a register with M = 5.
The yardsticks are timed in the same process on the same register, never constants:
  hadamard_gate(12)                      one launch that reads and writes every amplitude once (32 B per amplitude)
  c_amodc_gate(21, 2, control n - 1)     the closest kernel there was before (k_camodc), which skips the rows >= C
The new call:
  the twin          modmul_table(2, 21, 5) on (0, 5) under a control at n - 1: k_camodc's work plus the rows >= C
  uncontrolled      (0,5) (0,12) (3,9) (8,4) (12,8) (18,12) (26,4): whole-line tiles, the same bytes as the Hadamard
                    (1,12) (2,11) (5,10): tiles that share lines with their neighbours (num >= 10, first > 0)
  controlled (3,9)  one, two and three controls at bits >= 3 (squeezed: traffic 2^-k), one control at bit 0 (a predicate),
                    the latter also with perm_store_all = 0
  perm_nt = 1       nontemporal stores, on (0,5), (3,9), (12,8) and the twin
  perm_tile_log2    tiles of 2^8 and 2^10 amplitudes instead of the default's 2^12, on (0,5), (8,4), (26,4) and the twin
And, once, what the call replaces: the 6-bit adder k -> k + 17 mod 61 on (3, 6) as a network of X gates under five controls
through mc_one_qubit_gate (every transposition of the table a Gray-code walk), checked on the host against the table.
HIP events on the register's stream (timer_start / timer_stop) around each case.  The cases alternate, `--reps` rounds after a
warm-up call of each; the Hadamard is in every round TWICE, and the two series, identical work, give the run's own spread.
All rows are timed in ONE child process under `timeout`.  One JSON object per line, on stdout and in --out.

  python tools/time_permutation_gate.py [--n 30] [--reps 9] [--out profiles/permutation_gate_n30_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"perm_nt": 0, "perm_store_all": 1, "perm_tile_log2": 12}


def toffoli_network(table, num):
    """[(bit, {control: value})]: X gates under num - 1 controls whose product, in order, is the table"""
    inv = np.empty(1 << num, dtype=np.int64)
    inv[np.asarray(table, dtype=np.int64)] = np.arange(1 << num)
    p = list(range(1 << num))                                        # the image of every source so far
    gates = []
    for t in range(1 << num):
        s = int(inv[t])
        a = p[s]
        if a == t:
            continue
        path = [a]                                                   # a Gray-code walk from a to t
        for b in range(num):
            if (path[-1] ^ t) >> b & 1:
                path.append(path[-1] ^ (1 << b))
        steps = list(zip(path, path[1:]))
        for x, y in steps + steps[-2::-1]:                           # there, and back without the last step: the transposition (a t)
            b = (x ^ y).bit_length() - 1
            gates.append((b, {c: (x >> c) & 1 for c in range(num) if c != b}))
        p = [t if v == a else (a if v == t else v) for v in p]
    # on the host: the network is the table
    q = list(range(1 << num))
    for b, ctl in gates:
        q = [v ^ (1 << b) if all((v >> c) & 1 == val for c, val in ctl.items()) else v for v in q]
    assert q == [int(v) for v in table], "the network is not the table"
    return gates


def step(n, reps, out, network):
    sys.path.insert(0, ROOT)
    import quantumcomputer_amd as qc
    rs = np.random.RandomState(19)
    M = 5
    top = n - 1
    rows = []
    with qc.Register(n - M, M) as reg:
        reg.fill_random(30)
        reg.synchronize()
        yard = min(12, n - 1)
        twin_table = qc.modmul_table(2, 21, 5)
        plain = [s for s in [(0, 5), (0, 12), (3, 9), (8, 4), (12, 8), (18, 12), (26, 4), (1, 12), (2, 11), (5, 10)] if s[0] + s[1] <= n]
        tables = {s: rs.permutation(1 << s[1]) for s in plain}

        def hadamard():
            qc.hadamard_gate(yard, reg)

        def camodc():
            qc.c_amodc_gate(21, 2, top, reg)

        def perm_call(first, num, table, controls, knobs):
            cm = sum(1 << c for c in controls)
            cv = sum(1 << c for c, v in controls.items() if v)

            def f():
                if knobs:
                    qc.tune(**knobs)
                qc.permutation_gate(first, num, table, reg, controls=cm, values=cv)
                if knobs:
                    qc.tune(**{k: DEFAULTS[k] for k in knobs})
            return f

        # (label, first, num, table, controls, knobs)
        cases = [("twin_of_c_amodc", 0, 5, twin_table, {top: 1}, {})]
        cases += [(f"plain_{f}_{k}", f, k, tables[(f, k)], {}, {}) for f, k in plain]
        t39 = tables[(3, 9)]
        cases += [("controlled_3_9_c20", 3, 9, t39, {20: 1}, {}), ("controlled_3_9_c20_c21", 3, 9, t39, {20: 1, 21: 0}, {}),
                  ("controlled_3_9_c20_c21_c22", 3, 9, t39, {20: 1, 21: 0, 22: 1}, {}), ("controlled_3_9_c12_c13_c14", 3, 9, t39, {12: 1, 13: 1, 14: 1}, {}),
                  ("controlled_3_9_c0", 3, 9, t39, {0: 1}, {}), ("controlled_3_9_c0_no_store_all", 3, 9, t39, {0: 1}, {"perm_store_all": 0})]
        for lg in (8, 10):                                           # smaller tiles than the default's 2^12
            cases += [(f"twin_of_c_amodc_tile{lg}", 0, 5, twin_table, {top: 1}, {"perm_tile_log2": lg})]
            cases += [(f"plain_{f}_{k}_tile{lg}", f, k, tables[(f, k)], {}, {"perm_tile_log2": lg}) for f, k in [(0, 5), (8, 4), (26, 4)]]
        cases += [("twin_of_c_amodc_nt", 0, 5, twin_table, {top: 1}, {"perm_nt": 1})]
        cases += [(f"plain_{f}_{k}_nt", f, k, tables[(f, k)], {}, {"perm_nt": 1}) for f, k in [(0, 5), (3, 9), (12, 8)]]
        fs = [hadamard, camodc] + [perm_call(*c[1:]) for c in cases] + [hadamard]
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
        cmed = statistics.median(ts[1])
        rows.append({"case": "c_amodc_gate_21_2", "n": n, "M": M, "control": top, "median_ms": round(cmed, 4), "min_ms": round(min(ts[1]), 4),
                     "max_ms": round(max(ts[1]), 4), "ratio_to_hadamard": round(cmed / med, 4)})
        for (label, first, num, table, controls, knobs), t in zip(cases, ts[2:-1]):
            cm = sum(1 << c for c in controls)
            cv = sum(1 << c for c, v in controls.items() if v)
            if knobs:
                qc.tune(**knobs)
            pl = qc.permutation_plan(n, cm, cv, first, num)[1]
            if knobs:
                qc.tune(**{k: DEFAULTS[k] for k in knobs})
            m = statistics.median(t)
            fires = (1 << n) >> len(controls)
            row = {"case": label, "n": n, "first": first, "num": num, "controls": {str(c): v for c, v in controls.items()}, "knobs": knobs,
                   "form": ["lines", "shared"][pl.form], "kernel": pl.kernel.decode(), "T": pl.T, "units": int(pl.units), "grid": pl.grid,
                   "block": pl.block, "lds_bytes": pl.lds_bytes, "store_all": pl.store_all,
                   "median_ms": round(m, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                   "ratio_to_hadamard": round(m / med, 4), "bytes_moved": 32 * fires, "tb_per_s": round(32 * fires / 1e9 / m, 3)}
            if label.startswith("twin"):
                row["ratio_to_c_amodc"] = round(m / cmed, 4)
            rows.append(row)
        if network:
            table = qc.modadd_table(17, 6, modulus=61)
            gates = toffoli_network(table, 6)
            X = np.array([[0, 1], [1, 0]], dtype=complex)
            first = 3
            b, ctl = gates[0]
            qc.mc_one_qubit_gate([c + first for c in ctl], b + first, X, reg, values={c + first: v for c, v in ctl.items()})      # warm-up
            reg.timer_start()
            for b, ctl in gates:
                qc.mc_one_qubit_gate([c + first for c in ctl], b + first, X, reg, values={c + first: v for c, v in ctl.items()})
            t = reg.timer_stop()
            reg.timer_start(); qc.permutation_gate(first, 6, table, reg); t1 = reg.timer_stop()
            rows.append({"case": "modadd_17_mod_61_as_x_gates_under_5_controls", "n": n, "first": first, "num": 6, "gates": len(gates),
                         "ms": round(t, 2), "samples": 1, "permutation_gate_ms": round(t1, 4)})
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
    ap.add_argument("--no-network", action="store_true", help="skip the adder as a network of X gates under five controls (hundreds of launches)")
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", help="JSON lines are appended here (default: profiles/permutation_gate_n<n>_timing.jsonl, started afresh)")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        step(a.n, a.reps, a.out, not a.no_network)
        return 0
    out = a.out
    if not out:
        out = os.path.join(ROOT, "profiles", f"permutation_gate_n{a.n}_timing.jsonl")
        open(out, "w").close()
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
           "--n", str(a.n), "--reps", str(a.reps), "--out", out, "--step"] + (["--no-network"] if a.no_network else [])
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(json.dumps({"error": f"exit status {rc}"}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
