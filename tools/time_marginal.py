#!/usr/bin/env python3
"""Cost of qcx_marginal_probabilities (DESIGN s4.5d) on one GPU: a dense fill_random state -- the L-register range
(first = 5, num = n - 5), the M-register range (first = 0, num = 5) and num = 0 -- and the Shor N = 21, a = 2 state (M = 5,
its result left compact and read in place): the whole L register, and its top 5 qubits (a small output: no copy to speak of).  Every step runs in a child process of its own under `timeout`, so a
step that hangs ends there and nothing else starts on the GPU after a failed step.  device_ms = HIP events on the register's
stream around the call: the stages AND the copy of the output to the host (none for the Shor case: recording an event flushes,
which would expand the compact result); wall_ms = host clock around the call (it returns with the output on the host);
copy_mib = the output's size.
The kernels alone: a rocprofv3 kernel trace of one step (--step CASE).  The best of `--reps`.  One JSON object per case on stdout.

  python tools/time_marginal.py [--n 30] [--reps 5] [--step-timeout 600]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("dense_L", "dense_M", "dense_0", "shor_L", "shor_top5")


def step(case, n, reps):
    sys.path.insert(0, ROOT)
    import quantumcomputer_amd as qc
    M = 5
    first, num = {"dense_L": (M, n - M), "dense_M": (0, M), "dense_0": (0, 0), "shor_L": (M, n - M), "shor_top5": (n - 5, 5)}[case]
    shor = case.startswith("shor")
    best_dev = best_wall = float("inf")
    with qc.Register(n - M, M) as reg:
        def prepare():
            if shor:                                    # (no synchronize here: it flushes, i.e. expands the compact result)
                qc.reset_register(reg)
                qc.quantum_computation(21, 2, reg)
            else:
                reg.fill_random(30)
                reg.synchronize()
        prepare()
        reg.marginal(first, num)                        # warm-up: the scratch, the code objects
        for _ in range(reps):
            prepare()
            if shor:
                # the first call runs the circuit's deferred last pass (the state stays compact); the second, timed, reads the
                # compact form alone.  No HIP events here: recording one flushes, i.e. expands the compact result.
                reg.marginal(first, num)
                t0 = time.perf_counter()
                reg.marginal(first, num)
                best_wall = min(best_wall, time.perf_counter() - t0)
                continue
            reg.timer_start()
            t0 = time.perf_counter()
            reg.marginal(first, num)
            wall = time.perf_counter() - t0
            dev = reg.timer_stop()
            best_dev, best_wall = min(best_dev, dev), min(best_wall, wall)
        src, reads = reg.marginal_stats()
    state_gb = (16 << n) / 1e9
    print(json.dumps({"case": case, "n": n, "first": first, "num": num, "source": src, "state_reads": reads,
                      "device_ms": round(best_dev, 4) if best_dev < float("inf") else None, "wall_ms": round(best_wall * 1e3, 4),
                      "copy_mib": (8 << num) / 2**20,
                      "state_tb_per_s": round(state_gb / best_dev, 3) if best_dev < float("inf") else None}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--step", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        step(a.step, a.n, a.reps)
        return 0
    for case in a.cases.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
               "--n", str(a.n), "--reps", str(a.reps), "--step", case]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(json.dumps({"case": case, "error": f"exit status {rc}"}), flush=True)
            return rc                                   # nothing more on the GPU after a failed step
    return 0


if __name__ == "__main__":
    sys.exit(main())
