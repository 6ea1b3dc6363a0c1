"""The circuits of the TOLERANCE MODE tests (tests/test_gpu_tolerance_mode.py) as data: shapes, seeds and gate lists in the step
form of tests/exact_ref.py, so that the GPU tests, the CPU tests of the criterion (tests/test_exact_ref.py) and
tools/measure_tolerance_accuracy.py speak of the same cases.  Host only."""
import math

import numpy as np

IQFT_SHAPES = [(10, 0), (12, 0), (14, 4), (16, 0), (16, 5), (11, 5)]          # (n, M), fill_random(IQFT_SEED)
IQFT_SEED = 21
IQFT_GEOMS = [None, (10, 4), (11, 4), (12, 3), (12, 4)]
IQFT_GEOM_IDS = ["default", "T10c4", "T11c4", "T12c3", "T12c4"]
SHOR_SHAPES = [(15, 3, 4, 7), (15, 8, 4, 7), (21, 9, 5, 2), (35, 6, 6, 2), (21, 11, 5, 2)]      # (C, L, M, a), the reset state
RADIX8_SHAPES = [(12, 0), (12, 3), (20, 0), (21, 5), (24, 0), (20, 4)]      # (n, M), fill_random(RADIX8_SEED)
RADIX8_SEED = 8
RADIX8_TRUTH_MAX_N = 20                       # above it a long-double truth does not fit a test: the old bound alone
SWITCH_SHAPE, SWITCH_SEED = (14, 0), 4
PROGRAM_SEEDS = range(8)


def random_program(seed):
    """test_random_programs_within_tolerance: (n, M, C, knobs, steps), input fill_random(seed).  Phase runs that share a qubit
    (targets may repeat), phases that share none, Hadamards, modular multiplies; controls on register bits, lane bits and
    outside the tile; several geometries and a grid that walks many tiles"""
    rs = np.random.RandomState(300 + seed)
    n, M = int(rs.randint(10, 19)), int(rs.choice([0, 3, 4, 5]))
    Cn = int(rs.randint(3, 1 << M)) if M else 1
    T, c = [(10, 4), (11, 4), (12, 3), (11, 2), (12, 4), (10, 6), (11, 4), (12, 0)][seed]
    knobs = dict(fuse_T=min(T, n), fuse_c=min(c, T, n), fuse_grid_cap=[0, 5][seed % 2] or 24576, fuse_tol_T=[0, 10][seed % 2], fuse_q3=[1, 0, 1, 1][seed % 4])
    steps = []
    for _ in range(int(rs.randint(30, 70))):
        k = rs.randint(0, 10)
        if k < 3:
            steps.append(("h", int(rs.randint(0, n))))
        elif k < 8 or M == 0:
            ctl = int(rs.randint(0, n))
            for _ in range(int(rs.randint(1, 10))):
                t = int(rs.randint(0, n))
                if t == ctl:
                    continue
                steps.append(("p", ctl, t, float(rs.uniform(-3, 3))))
        else:
            atox, ctl = int(rs.randint(1, 4 * Cn)), int(rs.randint(M, n))
            steps.append(("c", Cn, atox, ctl))
    return n, M, Cn, knobs, steps


# ---- run-merge edges on a 13-qubit register ----------------------------------------------------------------------------------
# Hadamards on qubits 11 .. 5, then H(12) and ONE run of controlled phases on the top qubit: the last round of the pass carries
# the merged diagonal, and nothing mixes the amplitudes behind it.  Under the default knobs the pass runs on a 2^12 tile made of
# qubits 0-3 and 5-12 (tests/test_fusion_plan.py pins that), the control is tile bit 11, and the three targets sit on
#     qubit 0   tile bit 0                                  -> its factor comes from table G0   (angle pi / 2)
#     qubit 11  tile bit 10, the highest beside the control -> G2                               (angle pi / 2^11)
#     qubit 4   the one bit outside the tile                -> the per-tile constant E_out      (angle pi / 2^12)
# so a wrong entry in one table shows in that target's half-space alone.
EDGE_N, EDGE_SEED = 13, 13
EDGE_CTL = EDGE_N - 1
EDGE_TARGETS = {"G0": (0, math.pi / 2), "G2": (11, math.pi / float(1 << 11)), "E_out": (4, math.pi / float(1 << 12))}
EDGE_KNOBS = [dict(), dict(fuse_q3=0), dict(fuse_x8t=0), dict(fuse_T=12, fuse_c=4, fuse_T_phase=0, fuse_tol_T=0, fuse_q3=0)]
EDGE_KNOB_IDS = ["default", "fuse_q3=0", "fuse_x8t=0", "T12c4-radix4"]
EDGE_KNOB_KEYS = sorted({k for d in EDGE_KNOBS for k in d})


def edge_steps():
    steps = [("h", q) for q in range(EDGE_N - 2, 4, -1)] + [("h", EDGE_CTL)]
    return steps + [("p", EDGE_CTL, t, th) for t, th in EDGE_TARGETS.values()]


def edge_half_spaces():
    """{table: the amplitudes its factor reaches}: control and target both set"""
    idx = np.arange(1 << EDGE_N)
    return {name: (((idx >> EDGE_CTL) & 1) == 1) & (((idx >> t) & 1) == 1) for name, (t, _) in EDGE_TARGETS.items()}


def apply_steps(qc, reg, steps):
    for s in steps:
        if s[0] == "h":
            qc.hadamard_gate(s[1], reg)
        elif s[0] == "p":
            qc.c_phase_shift_gate(s[1], s[2], s[3], reg)
        else:
            qc.c_amodc_gate(s[1], s[2], s[3], reg)


def oracle_steps(ob, state, n, M, steps, threads=8):
    for s in steps:
        if s[0] == "h":
            ob.hadamard(state, n, s[1], threads)
        elif s[0] == "p":
            ob.cphase(state, n, s[1], s[2], s[3], threads)
        else:
            ob.camodc(state, n, M, s[1], s[2], s[3], threads)
    return state


# ---- (oracle's state, truth, gate count) of each case: computed once, shared, never changed ------------------------------------

def _pair(ob, key, start, n, M, steps):
    import exact_ref as er

    def make():
        a = start()
        T = er.truth(a, n, M, steps)
        want = oracle_steps(ob, a, n, M, steps)
        want.setflags(write=False)
        return want, T, len(steps)
    return er.cached(key, make)


def iqft_case(ob, n, M, seed):
    import exact_ref as er
    return _pair(ob, ("iqft", n, M, seed), lambda: ob.fill_random(n, seed), n, M, er.iqft_steps(n, M))


def shor_case(ob, Cn, L, M, a):
    import exact_ref as er
    n = L + M
    return _pair(ob, ("shor", Cn, L, M, a), lambda: er.basis_state(n, 1), n, M, er.qcomp_steps(Cn, a, L, M))


def program_case(ob, seed):
    n, M, Cn, knobs, steps = random_program(seed)
    return _pair(ob, ("program", seed), lambda: ob.fill_random(n, seed), n, M, steps)


def edge_case(ob):
    return _pair(ob, ("edge",), lambda: ob.fill_random(EDGE_N, EDGE_SEED), EDGE_N, 0, edge_steps())


def steps_case(ob, key, start, n, M, steps):
    """any other gate list: start() makes the input pairs"""
    return _pair(ob, key, start, n, M, steps)
