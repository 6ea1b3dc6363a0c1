#!/usr/bin/env python3
"""Cost of qcx_gate_batch (K12b / K13b, DESIGN s4.5l) on one GPU, dense fill_random state of n qubits, against the same list issued
gate by gate through qcx_one_qubit_gate / qcx_c_one_qubit_gate / qcx_two_qubit_gate / qcx_c_two_qubit_gate (one launch, one read
and one write of the state, or of its control-set half, per gate) and against the yardstick hadamard_gate(12), all timed in the
same process on the same register.  The lists:
  low32     32 one-qubit gates on qubits 0-7: one pass, every gate exchanges between threads (inside the wave, or through LDS)
  hot4      4 one-qubit gates on qubits 12-15: one pass, registers only
  ansatz    a hardware-efficient layer: ry on every qubit, then CNOT(q, q + 1) along the chain
  qft12     the forward QFT of 12 qubits placed at qubits 9-20, as H plus c_one_qubit_gate(phase(theta))
  bonds10   10 random two-qubit unitaries on bonds inside qubits 8-11: one pass, registers only
Each list is a `batch` row and a `gate_by_gate` row; ansatz and qft12 also give one row per PASS of their plan (the pass's gates as
a list of their own, which plans to the same single pass).  A batch row carries what its passes move and compute:
traffic_tb_per_s = passes * 32 B * 2^n / time, and fp64_issue_fraction = the FP64 wave-instructions per SIMD the gates need (16 per
amplitude for a one-target row, 32 for a two-target row, half of that under a control; 64 amplitudes to an instruction, --simds
SIMDs) times the measured 2.18 ns each (DESIGN s8), over the time: 1.0 is the issue ceiling.
HIP events on the register's stream around each case.  The cases alternate, `--reps` rounds after a warm-up call of each; the
Hadamard is in every round TWICE, and the two series, identical work, give the run's own spread.  All rows are timed in ONE child
process under `timeout`.  One JSON object per line, on stdout and in --out.

  python tools/time_gate_batch.py [--n 30] [--reps 9] [--out profiles/gate_batch_n30_timing.jsonl]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP64_NS = 2.18


def random_unitary(np, seed, d):
    rs = np.random.RandomState(seed)
    q, r = np.linalg.qr(rs.randn(d, d) + 1j * rs.randn(d, d))
    u = q * (np.diag(r) / np.abs(np.diag(r)))
    return np.clip(u.real, -1.0, 1.0) + 1j * np.clip(u.imag, -1.0, 1.0)


def ry(np, theta):
    c, s = math.cos(theta / 2), math.sin(theta / 2)
    return np.array([[c, -s], [s, c]], dtype=complex)


def lists(qc, np, n):
    """gates as gate_batch takes them: (U, targets) or (U, targets, control)"""
    low = min(8, n)
    h0 = max(0, min(12, n - 4))
    b0 = max(0, min(8, n - 4))
    q0 = max(0, min(9, n - 12))
    nq = min(12, n)
    qft = []
    for t in range(q0 + nq - 1, q0 - 1, -1):                         # H on the target, then the phases onto it from the qubits below
        qft.append((qc.GATES["H"], t))
        qft += [(qc.phase(math.pi / (1 << (t - c))), t, c) for c in range(t - 1, q0 - 1, -1)]
    return [("low32", [(random_unitary(np, k, 2), k % low) for k in range(32)]),
            ("hot4", [(random_unitary(np, 40 + k, 2), h0 + k) for k in range(4)]),
            ("ansatz", [(ry(np, 0.1 + 0.07 * q), q) for q in range(n)] + [(qc.GATES2["CNOT"], (q, q + 1)) for q in range(n - 1)]),
            ("qft12", qft),
            ("bonds10", [(random_unitary(np, 50 + k, 4), (b0 + k % 3, b0 + 1 + k % 3)) for k in range(10)])]


def targets_of(g):
    return (g[1],) if isinstance(g[1], int) else tuple(g[1])


def step(n, reps, out, simds):
    sys.path.insert(0, ROOT)
    import numpy as np
    import quantumcomputer_amd as qc
    cases = []                                                       # (name, kind, gates, hot masks)
    for name, gates in lists(qc, np, n):
        pass_of, hots = qc.gate_batch_plan(gates, n)
        cases.append((name, "batch", gates, hots))
        cases.append((name, "gate_by_gate", gates, None))
        if name in ("ansatz", "qft12"):
            for p in range(len(hots)):
                sub = [g for g, q in zip(gates, pass_of) if q == p]
                assert qc.gate_batch_plan(sub, n)[1] == [hots[p]]
                cases.append((f"{name}_pass_{p}", "batch", sub, [hots[p]]))
    rows = []
    with qc.Register(n, 0) as reg:
        reg.fill_random(30)
        reg.synchronize()
        yard = min(12, n - 1)

        def hadamard():
            qc.hadamard_gate(yard, reg)

        def batch(gates):
            return lambda: qc.gate_batch(gates, reg)

        def loop(gates):
            def f():
                for g in gates:
                    t = targets_of(g)
                    if len(t) == 1:
                        qc.one_qubit_gate(t[0], g[0], reg) if len(g) == 2 else qc.c_one_qubit_gate(g[2], t[0], g[0], reg)
                    else:
                        qc.two_qubit_gate(t[0], t[1], g[0], reg) if len(g) == 2 else qc.c_two_qubit_gate(g[2], t[0], t[1], g[0], reg)
            return f

        fs = [hadamard] + [batch(g) if kind == "batch" else loop(g) for _, kind, g, _ in cases] + [hadamard]
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
        med_of, range_of = {}, {}
        for (name, kind, gates, hots), t in zip(cases, ts[1:-1]):
            m = med_of[name, kind] = statistics.median(t)
            range_of[name, kind] = (min(t), max(t))
            row = {"case": name, "kind": kind, "n": n, "gates": len(gates), "median_ms": round(m, 4), "min_ms": round(min(t), 4),
                   "max_ms": round(max(t), 4), "ratio_to_hadamard": round(m / med, 4)}
            if kind == "batch":
                instr = sum((16 if len(targets_of(g)) == 1 else 32) * (0.5 if len(g) == 3 else 1.0) for g in gates) * (1 << n) / 64 / simds
                row.update({"passes": len(hots), "hot_masks": hots, "lds_gates": sum(1 for g in gates if min(targets_of(g)) < 8),
                            "ms_per_pass": round(m / len(hots), 4), "traffic_tb_per_s": round(len(hots) * gb / m, 3),
                            "fp64_wave_instructions_per_simd": round(instr), "fp64_issue_fraction": round(instr * FP64_NS * 1e-6 / m, 3)})
            else:
                b_lo, b_hi = range_of[name, "batch"]
                row.update({"passes": len(gates), "batch_speedup": round(m / med_of[name, "batch"], 3),
                            "batch_is_not_slower": bool(med_of[name, "batch"] <= m),
                            "ranges_overlap": bool(b_hi >= min(t))})
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
    ap.add_argument("--out", help="JSON lines are appended here (default: profiles/gate_batch_n<n>_timing.jsonl, started afresh)")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        step(a.n, a.reps, a.out, a.simds)
        return 0
    out = a.out
    if not out:
        out = os.path.join(ROOT, "profiles", f"gate_batch_n{a.n}_timing.jsonl")
        open(out, "w").close()
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
           "--n", str(a.n), "--reps", str(a.reps), "--simds", str(a.simds), "--out", out, "--step"]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(json.dumps({"error": f"exit status {rc}"}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
