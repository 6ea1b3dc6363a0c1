#!/usr/bin/env python3
"""Cost of qcx_sample_states (DESIGN s4.5c) on one GPU: K = 1, 64, 1024, 16384 shots from one n-qubit state -- a dense
fill_random state and the Shor N = 21, a = 2 state (M = 5, its result left compact) -- next to one measure_state on the same
state.  Every step runs in a child process of its own under `timeout`, so a step that hangs ends there and nothing else
starts on the GPU after a failed step.  Times are host wall clock around calls that synchronise the device (sample_states
and measure_state wait for their result); the best of `--reps`.  One JSON object per step on stdout.

  python tools/time_samples.py [--n 30] [--reps 5] [--step-timeout 600]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHOTS = (1, 64, 1024, 16384)


def prepare(qc, reg, kind):
    if kind == "dense":
        reg.fill_random(30)
    else:
        qc.reset_register(reg)
        qc.quantum_computation(21, 2, reg)
    reg.synchronize()


def step(kind, what, n, reps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import quantumcomputer_amd as qc
    L, M = (n, 0) if kind == "dense" else (n - 5, 5)
    best = float("inf")
    with qc.Register(L, M) as reg:
        if what == "measure":
            for i in range(reps + 1):
                prepare(qc, reg, kind)
                t0 = time.perf_counter()
                qc.measure_state(reg, 0.3 + 0.1 * i)
                dt = time.perf_counter() - t0
                if i:                                   # (the first call allocates the scan's scratch)
                    best = min(best, dt)
            stats = None
        else:
            k = int(what)
            rs = np.random.RandomState(k).uniform(0, 1, k)
            prepare(qc, reg, kind)
            qc.sample_states(reg, rs)                   # warm-up: allocations
            for _ in range(reps):
                reg.synchronize()
                t0 = time.perf_counter()
                qc.sample_states(reg, rs)
                best = min(best, time.perf_counter() - t0)
            stats = reg.sample_stats()
    out = {"state": kind, "n": n, "call": "measure_state" if what == "measure" else "sample_states",
           "shots": 1 if what == "measure" else int(what), "ms": round(best * 1e3, 4)}
    if stats is not None:
        out["state_scans"], out["fallback_shots"] = stats
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--step", nargs=2, metavar=("STATE", "WHAT"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        step(a.step[0], a.step[1], a.n, a.reps)
        return 0
    for kind in ("dense", "shor"):
        for what in ["measure"] + [str(k) for k in SHOTS]:
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
                   "--n", str(a.n), "--reps", str(a.reps), "--step", kind, what]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(json.dumps({"state": kind, "step": what, "error": f"exit status {rc}"}), flush=True)
                return rc                               # nothing more on the GPU after a failed step
    return 0


if __name__ == "__main__":
    sys.exit(main())
