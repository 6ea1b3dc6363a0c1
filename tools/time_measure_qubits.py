#!/usr/bin/env python3
"""Cost of qcx_measure_qubits (DESIGN s4.5e) on one GPU, dense fill_random state of n qubits, for the ranges (12, 4), (0, 2),
(5, n - 5) = the L register, (0, 5) = the M register and (n - 1, 1).  Per range, all in ONE process and on one register:
  hadamard12_ms   one qcx_hadamard_gate(12) launch (32 * 2^n bytes moved): the yardstick
  collapse_ms     the collapse pass alone (k_collapse_range through the diagnostic entry qcx_collapse_pass)
  marginal_ms     qcx_marginal_probabilities on the range (its stages and the copy of 2^num doubles to the host)
  call_ms         the whole qcx_measure_qubits_r call between two HIP events: marginal, the host's scan of P, collapse pass
  call_wall_ms    the same call on the host clock
HIP events on the register's stream (timer_start / timer_stop), the best of `--reps` after a warm-up call of each.  Every range
runs in a child process of its own under `timeout`; nothing more starts on the GPU after a failed step.  One JSON object per
range on stdout.  --grid-cap / --perm / --upt set the kernel's launch knobs (sweeps).

  python tools/time_measure_qubits.py [--n 30] [--reps 5] [--step-timeout 300]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ranges(n):
    return [(12, 4), (0, 2), (5, n - 5), (0, 5), (n - 1, 1)]


def step(first, num, n, reps, grid_cap, perm, upt):
    sys.path.insert(0, ROOT)
    import quantumcomputer_amd as qc
    from quantumcomputer_amd._lib import check, lib
    if grid_cap is not None:
        qc.tune(collapse_grid_cap=grid_cap)
    if perm is not None:
        qc.tune(collapse_perm=perm)
    if upt is not None:
        qc.tune(collapse_upt=upt)
    M = 5
    best = {k: float("inf") for k in ("hadamard12_ms", "collapse_ms", "marginal_ms", "call_ms", "call_wall_ms")}

    def timed(key, fn):
        reg.timer_start()
        fn()
        best[key] = min(best[key], reg.timer_stop())

    with qc.Register(n - M, M) as reg:
        reg.fill_random(30)
        reg.synchronize()
        hq = min(12, n - 1)
        qc.hadamard_gate(hq, reg)                                   # warm-up of each: code objects, scratch
        reg.marginal(first, num)
        check(lib().qcx_collapse_pass(reg._h, first, num, 0, 1.0), "qcx_collapse_pass")
        for _ in range(reps):
            reg.fill_random(30)
            reg.synchronize()
            timed("hadamard12_ms", lambda: qc.hadamard_gate(hq, reg))
            timed("marginal_ms", lambda: reg.marginal(first, num))
            reg.timer_start()
            t0 = time.perf_counter()
            outcome, p = reg.measure_qubits(first, num, 0.5)
            best["call_wall_ms"] = min(best["call_wall_ms"], (time.perf_counter() - t0) * 1e3)
            best["call_ms"] = min(best["call_ms"], reg.timer_stop())
            # the pass alone, on the collapsed state (s = 1: the kept amplitudes keep their values; the time does not depend on them)
            timed("collapse_ms", lambda: check(lib().qcx_collapse_pass(reg._h, first, num, outcome, 1.0), "qcx_collapse_pass"))
        stats = reg.collapse_stats()
    moved = (16 << n) + (16 << (n - num))                           # bytes the pass must move when whole lines are dropped
    out = {"n": n, "first": first, "num": num, "outcome": outcome, "probability": p, "stats": list(stats)}
    out.update({k: round(v, 4) for k, v in best.items()})
    out["collapse_over_hadamard"] = round(best["collapse_ms"] / best["hadamard12_ms"], 4)
    out["collapse_tb_per_s"] = round(moved / 1e9 / best["collapse_ms"], 3)
    out["copy_mib"] = (8 << num) / 2**20
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--grid-cap", type=int)
    ap.add_argument("--perm", type=int)
    ap.add_argument("--upt", type=int)
    ap.add_argument("--ranges", help="first:num,first:num,... (default: the five ranges of DESIGN s4.5e)")
    ap.add_argument("--step", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        first, num = (int(x) for x in a.step.split(":"))
        step(first, num, a.n, a.reps, a.grid_cap, a.perm, a.upt)
        return 0
    rl = [tuple(int(x) for x in s.split(":")) for s in a.ranges.split(",")] if a.ranges else ranges(a.n)
    for first, num in rl:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
               "--n", str(a.n), "--reps", str(a.reps), "--step", f"{first}:{num}"]
        if a.grid_cap is not None:
            cmd += ["--grid-cap", str(a.grid_cap)]
        if a.perm is not None:
            cmd += ["--perm", str(a.perm)]
        if a.upt is not None:
            cmd += ["--upt", str(a.upt)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(json.dumps({"first": first, "num": num, "error": f"exit status {rc}"}), flush=True)
            return rc                                               # nothing more on the GPU after a failed step
    return 0


if __name__ == "__main__":
    sys.exit(main())
