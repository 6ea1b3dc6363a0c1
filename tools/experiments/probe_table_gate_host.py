#!/usr/bin/env python3
"""One-off probe: the host time of a call of the five masked and table gates (qcx_mc_one_qubit_gate, qcx_mc_two_qubit_gate,
qcx_diagonal_gate, qcx_permutation_gate, qcx_mc_multi_qubit_gate) where the kernels are launch-bound: n = 12.  Per gate,
`--reps` samples of `--calls` back-to-back calls through the C ABI with arguments built beforehand, a host clock around the loop
and the synchronise that ends it; microseconds per call.  The mc gates carry one positive and one negative control, so that
they take K17's path; the multi-qubit gate has three targets; the tables change nothing about the cost.  One JSON object per
line, on stdout and appended to --out; --run labels the rows (the build the library was made from).

  python tools/experiments/probe_table_gate_host.py [--n 12] [--calls 2000] [--reps 7] [--run NAME] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=12)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--run", default="")
    ap.add_argument("--out")
    a = ap.parse_args()
    import quantumcomputer_amd as qc
    L = qc.lib()
    rs = np.random.RandomState(1)
    H = np.array([1, 0, 1, 0, 1, 0, -1, 0], dtype=np.float64) * 0.5 ** 0.5
    sw = np.zeros(32); sw[[0, 12, 18, 30]] = 1.0                                    # SWAP
    d = np.exp(1j * rs.uniform(0, 6, 1 << 6)).view(np.float64)
    perm = rs.permutation(1 << 4).astype(np.uint32)
    q, _ = np.linalg.qr(rs.randn(8, 8) + 1j * rs.randn(8, 8))
    u3 = np.ascontiguousarray(np.clip(q.real, -1, 1) + 1j * np.clip(q.imag, -1, 1)).reshape(-1).view(np.float64)
    t3 = (C.c_uint * 3)(1, 6, 9)
    pH, pS, pD, pP, pU = (arr.ctypes.data_as(C.c_void_p) for arr in (H, sw, d, perm, u3))
    pT = C.cast(t3, C.c_void_p)
    cm, cv = (1 << 5) | (1 << 7), 1 << 5
    with qc.Register(a.n, 0) as reg:
        h = reg._h
        gates = {
            "qcx_mc_one_qubit_gate": lambda: L.qcx_mc_one_qubit_gate(cm, cv, 3, pH, h),
            "qcx_mc_two_qubit_gate": lambda: L.qcx_mc_two_qubit_gate(cm, cv, 2, 9, pS, h),
            "qcx_diagonal_gate": lambda: L.qcx_diagonal_gate(3, 6, pD, h),
            "qcx_permutation_gate": lambda: L.qcx_permutation_gate(cm, cv, 8, 4, pP, h),
            "qcx_mc_multi_qubit_gate": lambda: L.qcx_mc_multi_qubit_gate(cm, cv, 3, pT, pU, h),
        }
        for name, call in gates.items():
            reg.fill_random(3)
            assert call() == 0, (name, L.qcx_last_error())
            reg.synchronize()
            us = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    call()
                reg.synchronize()
                us.append(1e6 * (time.perf_counter() - t0) / a.calls)
            row = {"run": a.run, "tool": f"tools/experiments/probe_table_gate_host.py --n {a.n}", "case": name, "n": a.n, "calls": a.calls,
                   "reps": a.reps, "median_us": round(statistics.median(us), 3), "min_us": round(min(us), 3), "max_us": round(max(us), 3)}
            line = json.dumps(row)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
