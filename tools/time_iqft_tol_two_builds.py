#!/usr/bin/env python3
"""Two builds of libqcx.so in ONE process, alternately: the n = 28 inverse QFT in the tolerance mode (qcx_set_fusion(reg, 2)), and
the same followed by a switch to mode 0 and one hadamard_gate -- the first exact gate behind a tolerance flush, which runs the
zero pass such a flush leaves owed.  HIP events of each build's own qcx_timer_*; one JSON line per row.

    python tools/time_iqft_tol_two_builds.py NAME_A=path/to/libqcx.so NAME_B=path/to/other/libqcx.so [n] [rounds]
"""
import ctypes as C
import json
import os
import statistics
import sys


def load(path):
    lib = C.CDLL(os.path.abspath(path))
    p, i, u, d = C.c_void_p, C.c_int, C.c_uint, C.c_double
    for name, res, args in (("qcx_register_create", i, [i, i, C.POINTER(p)]), ("qcx_register_destroy", i, [p]), ("qcx_set_fusion", i, [p, i]),
                            ("qcx_state_fill_random", i, [p, C.c_uint64]), ("qcx_inverse_QFT", i, [p]), ("qcx_hadamard_gate", i, [u, p]),
                            ("qcx_timer_start", i, [p]), ("qcx_timer_stop", i, [p, C.POINTER(d)]), ("qcx_synchronize", i, [p])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def ok(st):
    if st != 0:
        raise RuntimeError(f"status {st}")


def timed(lib, reg, work):
    ms = C.c_double(0.0)
    ok(lib.qcx_timer_start(reg)); work(); ok(lib.qcx_timer_stop(reg, C.byref(ms)))
    return ms.value


def main():
    builds = [kv.split("=", 1) for kv in sys.argv[1:3]]
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 28
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 7
    libs = [(name, load(path)) for name, path in builds]
    regs = []
    for name, lib in libs:
        reg = C.c_void_p()
        ok(lib.qcx_register_create(n, 0, C.byref(reg)))
        ok(lib.qcx_state_fill_random(reg, 1))
        regs.append(reg)
    rows = {(name, what): [] for name, _ in libs for what in ("iqft_tolerance_ms", "iqft_tolerance_then_mode0_hadamard_ms")}
    for r in range(rounds + 1):                                            # (round 0 warms both builds up and is dropped)
        for (name, lib), reg in zip(libs, regs):
            def iqft():
                ok(lib.qcx_inverse_QFT(reg))
            def iqft_then_gate():
                ok(lib.qcx_inverse_QFT(reg)); ok(lib.qcx_set_fusion(reg, 0)); ok(lib.qcx_hadamard_gate(n - 1, reg))
            ok(lib.qcx_set_fusion(reg, 2))
            a = timed(lib, reg, iqft)
            b = timed(lib, reg, iqft_then_gate)
            if r:
                rows[(name, "iqft_tolerance_ms")].append(a)
                rows[(name, "iqft_tolerance_then_mode0_hadamard_ms")].append(b)
    for (name, what), v in rows.items():
        print(json.dumps({"row": what, "build": name, "n": n, "min": min(v), "median": statistics.median(v), "max": max(v), "runs": len(v)}), flush=True)
    for (name, lib), reg in zip(libs, regs):
        ok(lib.qcx_register_destroy(reg))


if __name__ == "__main__":
    main()
