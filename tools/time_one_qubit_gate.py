#!/usr/bin/env python3
"""Cost of qcx_one_qubit_gate / qcx_c_one_qubit_gate (K12, DESIGN s4.5f) on one GPU, dense fill_random state of n qubits.
  plain       per target q in {0, 2, 5, 8, 12, 21, n - 1}: one_qubit_ms (a seeded random unitary) against hadamard_ms, one
              qcx_hadamard_gate(q) launch timed in the same process on the same register -- the yardstick: both move
              32 * 2^n bytes.  ratio = one_qubit_ms / hadamard_ms (aim: <= 1.10).
  controlled  per (c, q): c_one_qubit_ms against phase_ms, one qcx_c_phase_shift_gate(c, q) launch; the gate moves the
              control-set half of the state (16 * 2^n bytes), twice the phase gate's bytes:
              ratio_per_byte = c_one_qubit_ms / (2 * phase_ms).  Pairs with c or q below 3 take the whole-line kernel.
HIP events on the register's stream (timer_start / timer_stop); the two launches of a row alternate, the best of `--reps` each
after a warm-up call of each.  The two steps run in child processes of their own under `timeout`; nothing more starts on the
GPU after a failed step.  One JSON object per line, on stdout and appended to --out.

  python tools/time_one_qubit_gate.py [--n 30] [--reps 7] [--out profiles/one_qubit_gate_n30_timing.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unitary(seed):
    import numpy as np
    rs = np.random.RandomState(seed)
    q, r = np.linalg.qr(rs.randn(2, 2) + 1j * rs.randn(2, 2))
    u = q * (np.diag(r) / np.abs(np.diag(r)))
    return np.clip(u.real, -1.0, 1.0) + 1j * np.clip(u.imag, -1.0, 1.0)


def targets(n):
    return sorted({q for q in (0, 2, 5, 8, 12, 21, n - 1) if q < n})


def pairs(n):
    top = n - 1
    want = [(top, 3), (3, top), (12, 21), (21, 12), (8, 5), (top - 1, top), (0, 12), (12, 0), (2, 1), (top, 0), (1, top)]
    return [(c, q) for c, q in want if c < n and q < n and c != q]


def step(kind, n, reps, out):
    sys.path.insert(0, ROOT)
    import math
    import quantumcomputer_amd as qc
    U = unitary(30)

    def best_of_both(reg, f, g):
        """the two launches alternate, so that both see the same neighbours and the same drift; best of `reps` each"""
        f(); g()                                                     # warm-up: code objects, launch path
        bf = bg = float("inf")
        for _ in range(reps):
            reg.timer_start(); f(); bf = min(bf, reg.timer_stop())
            reg.timer_start(); g(); bg = min(bg, reg.timer_stop())
        return bf, bg

    with qc.Register(n, 0) as reg:
        reg.fill_random(30)
        reg.synchronize()
        rows = []
        if kind == "plain":
            for q in targets(n):
                h, u = best_of_both(reg, lambda: qc.hadamard_gate(q, reg), lambda: qc.one_qubit_gate(q, U, reg))
                rows.append({"kind": kind, "n": n, "q": q, "hadamard_ms": round(h, 4), "one_qubit_ms": round(u, 4),
                             "ratio": round(u / h, 4), "one_qubit_tb_per_s": round((32 << n) / 1e9 / u, 3)})
        else:
            for c, q in pairs(n):
                theta = math.pi / 8
                p, u = best_of_both(reg, lambda: qc.c_phase_shift_gate(c, q, theta, reg), lambda: qc.c_one_qubit_gate(c, q, U, reg))
                rows.append({"kind": kind, "n": n, "c": c, "q": q, "form": "lines" if min(c, q) < 3 else "pair",
                             "phase_ms": round(p, 4), "c_one_qubit_ms": round(u, 4), "ratio_per_byte": round(u / (2 * p), 4),
                             "c_one_qubit_tb_per_s": round((16 << n) / 1e9 / u, 3)})
    for r in rows:
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", help="JSON lines are appended here (default: profiles/one_qubit_gate_n<n>_timing.jsonl, started afresh)")
    ap.add_argument("--step", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        step(a.step, a.n, a.reps, a.out)
        return 0
    out = a.out or os.path.join(ROOT, "profiles", f"one_qubit_gate_n{a.n}_timing.jsonl")
    open(out, "w").close()
    for kind in ("plain", "controlled"):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
               "--n", str(a.n), "--reps", str(a.reps), "--out", out, "--step", kind]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(json.dumps({"kind": kind, "error": f"exit status {rc}"}), flush=True)
            return rc                                               # nothing more on the GPU after a failed step
    return 0


if __name__ == "__main__":
    sys.exit(main())
