"""The calls of the four launch planners of the masked and the table gates (include/qcx_plan.h: qcx_mc_gate_plan,
qcx_diagonal_plan, qcx_permutation_plan, qcx_multi_gate_plan), enumerated, and the canonical line of one answer.
tests/test_table_gate_plans_pinned.py feeds the enumeration to the library and compares with the answers recorded from commit
14ef617, the one before the planners' checks, runs and tile geometry were stated once
(tests/golden/table_gate_plan_digests.json); the same module produced those, against that commit's own package:

    python tests/table_gate_plan_cases.py <checkout of 14ef617, built> > tests/golden/table_gate_plan_digests.json

A line is built from the plan's field names (FIELDS, in the order written here), never from the struct's bytes, so it does not
depend on the layout of a plan.  A refused call gives its status, and the text of qcx_last_error() where the refusal writes one:
a sentinel text is planted before the call, and a refusal that leaves it standing wrote none.
"""
import ctypes as C
import hashlib
import itertools
import json
import random
import sys

ENTRIES = ("mc", "diagonal", "permutation", "multi")

FIELDS = {
    "mc": ("form", "ns", "count", "nruns", "run_pos", "run_len", "or_const", "low_mask", "low_values", "store_all", "shfl_lo", "shfl_hi",
           "nt", "grid", "block", "items_per_thread", "glog", "slog", "kernel"),
    "diagonal": ("form", "full", "lds", "T", "first", "num", "kmask", "units", "elems", "slice_entries", "grid", "block", "lds_bytes",
                 "kernel"),
    "permutation": ("form", "T", "first", "num", "range_pos", "tile_bits", "tile_mask", "unit_mask", "squeezed", "or_const", "nruns",
                    "run_pos", "run_len", "elem_mask", "elem_values", "unit_mask_low", "unit_values_low", "units", "grid", "block",
                    "lds_bytes", "store_all", "nt", "kernel"),
    "multi": ("form", "T", "num_targets", "targets", "target_pos", "tile_bits", "tile_mask", "unit_mask", "squeezed", "or_const",
              "nruns", "run_pos", "run_len", "elem_mask", "elem_values", "unit_mask_low", "unit_values_low", "units", "grid", "block",
              "lds_bytes", "rows_per_item", "store_all", "nt", "kernel"),
}
ARRAYS = {"run_pos", "run_len", "tile_bits", "targets", "target_pos"}

# per entry point: the default knobs, and sets that move every knob its planner reads
KNOB_SETS = {
    "mc": {"default": {}, "ph_lines_0": {"ph_lines": 0}, "nt_0": {"ph_nt": 0, "u2_nt": 0}, "u2_variant_1": {"u2_variant": 1},
           "streams_3_0": {"ph_streams_log2": 3, "u2_streams_log2": 0}},
    "diagonal": {"default": {}, "lds_1": {"diag_lds": 1}, "grid_cap_7": {"diag_grid_cap": 7}, "grid_cap_0": {"diag_grid_cap": 0}},
    "permutation": {"default": {}, "tile_8": {"perm_tile_log2": 8}, "grid_cap_5": {"perm_grid_cap": 5},
                    "store_all_0_nt_1": {"perm_store_all": 0, "perm_nt": 1}},
    "multi": {"default": {}, "grid_cap_5": {"multi_grid_cap": 5}, "store_all_0_nt_1": {"multi_store_all": 0, "multi_nt": 1}},
}
KNOBS = sorted({k for sets in KNOB_SETS.values() for s in sets.values() for k in s})

# what the planners can answer: the forms, the kernel names and the refusal statuses (include/qcx.h: 2 = QCX_BAD_ARGUMENTS,
# 6 = QCX_BAD_QUBIT, 7 = QCX_UNSUPPORTED)
_B = ("true", "false")
FORMS = {"mc": {0, 1, 2, 3, 4}, "diagonal": {0, 1, 2}, "permutation": {0, 1}, "multi": {0}}
KERNELS = {
    "mc": {f"{k}<{b}>" for k in ("k_mcu_shfl", "k_mcu_pair", "k_mcu2_quad") for b in _B} | {f"k_mcu2_lines<{ns}, {b}>" for ns in (1, 2) for b in _B},
    "diagonal": {f"k_diagonal<{f}, {full}, false>" for f in (0, 1, 2) for full in _B} | {f"k_diagonal<2, {full}, true>" for full in _B},
    "permutation": {f"k_perm_tile<false, {b}>" for b in _B},
    "multi": {f"k_multi_tile<{k}, {b}>" for k in range(1, 6) for b in _B},
}
REFUSALS = {"mc": {2, 6, 7}, "diagonal": {2, 6}, "permutation": {2, 6}, "multi": {2, 6}}

NULL = "NULL"                  # as the last argument: a NULL `out`
NO_TARGETS = "NULL-targets"    # multi: a NULL `targets`
WIDE = (30, 33, 34, 40)


def _controls(others):
    """every assignment of the qubits `others` as no / positive / negative control: (mask, values)"""
    for pol in itertools.product(range(3), repeat=len(others)):
        cm = sum(1 << q for q, p in zip(others, pol) if p)
        yield cm, sum(1 << q for q, p in zip(others, pol) if p == 1)


def _drawn_controls(rng, n, opmask, must=()):
    """a seeded control assignment on the qubits outside opmask, of random density; the qubits `must` are controls"""
    dens = rng.choice((0.0, 0.1, 0.3, 0.6, 1.0))
    cm = sum(1 << q for q in range(n) if not (opmask >> q) & 1 and (q in must or rng.random() < dens))
    return cm, cm & rng.getrandbits(n)


def _special(n):
    """qubits 31, 32 and n - 1 where the register has them"""
    return [q for q in (31, 32, n - 1) if q < n]


def _target_cases(rng, ks, draws):
    """(n, mask, values, targets): exhaustive for n = 1 .. 6, then seeded draws"""
    for n in range(1, 7):
        for k in ks:
            for t in itertools.permutations(range(n), k):
                for cm, cv in _controls([q for q in range(n) if q not in t]):
                    yield n, cm, cv, t
    for n in (9, 10, 12, 13, 14) + WIDE:
        for d in range(draws):
            k = rng.choice([k for k in ks if k <= n])
            sp = _special(n) if n >= 30 else []
            low = list(range(min(n, 8)))
            # a third of the draws among the low qubits (the line forms), the wide ones with a special qubit as a target or a control
            pool = low if d % 3 == 0 else list(range(n))
            t = rng.sample(pool, k)
            free = [q for q in sp if q not in t]
            if free and d % 2:
                t[rng.randrange(k)] = rng.choice(free)
            opmask = sum(1 << q for q in t)
            cm, cv = _drawn_controls(rng, n, opmask, must=[q for q in sp if q not in t] if d % 4 < 2 else ())
            yield n, cm, cv, tuple(t)


def _range_cases(rng, draws, with_controls):
    """(n, mask, values, first, num): every range and control assignment for n = 1 .. 6, then seeded draws"""
    for n in range(1, 7):
        for first in range(n + 1):
            for num in range(n - first + 1):
                others = [q for q in range(n) if not first <= q < first + num]
                for cm, cv in (_controls(others) if with_controls else [(0, 0)]):
                    yield n, cm, cv, first, num
    for n in (9, 10, 12, 13, 14) + WIDE:
        for d in range(draws):
            num = rng.randrange(0, min(n, 12 if with_controls else 20) + 1)
            first = rng.randrange(0, n - num + 1)
            if n >= 30 and d % 2:               # the range on or next to qubits 31, 32, n - 1
                top = rng.choice(_special(n))
                first = max(0, min(n - num, top - rng.randrange(0, num + 1)))
            opmask = ((1 << num) - 1) << first
            cm, cv = _drawn_controls(rng, n, opmask, must=[q for q in _special(n) if not (opmask >> q) & 1] if n >= 30 and d % 4 < 2 else ())
            yield n, (cm if with_controls else 0), (cv if with_controls else 0), first, num


def cases(entry):
    """the enumeration of one entry point, in canonical order: a list of argument tuples (without `out`; NULL as the last element
    asks for a NULL `out`)"""
    rng = random.Random(f"table gate plans: {entry}")
    big = 0xFFFFFFFF
    if entry == "mc":
        out = [(n, cm, cv, len(t), t[0], t[1] if len(t) > 1 else 0) for n, cm, cv, t in _target_cases(rng, (1, 2), 600)]
        alt = sum(1 << q for q in range(3, 40, 2))          # 19 runs of squeezed positions
        out += [(12, 0, 0, 1, 0, 0, NULL), (12, 0, 0, 0, 0, 0), (12, 0, 0, 3, 0, 1), (0, 0, 0, 1, 0, 0), (41, 0, 0, 1, 0, 0),
                (12, 1, 3, 1, 4, 0), (12, 1, 3, 1, 12, 0), (12, 8, 24, 2, 4, 4), (12, 0, 0, 1, 12, 0), (12, 0, 0, 1, big, 0),
                (12, 0, 0, 2, 1, 12), (12, 0, 0, 2, 12, 1), (12, 0, 0, 2, 5, 5), (12, 1 << 12, 0, 1, 0, 0), (12, 1 << 63, 1 << 63, 1, 0, 0),
                (12, (1 << 64) - 1, 0, 1, 0, 0), (12, 1, 1, 1, 0, 0), (12, 6, 2, 2, 1, 7), (12, 6, 2, 2, 7, 2),
                (40, alt, alt, 1, 0, 0), (40, alt, 0, 2, 0, 2), (36, alt & ((1 << 36) - 1), 0, 1, 0, 0), (34, alt & ((1 << 34) - 1), 0, 1, 0, 0),
                (40, alt & ~(1 << 39), alt & 0xFF, 1, 39, 0)]
        return out
    if entry == "diagonal":
        out = [(n, first, num) for n, _, _, first, num in _range_cases(rng, 300, False)]
        out += [(n, first, num) for n in range(7, 15) for first in range(n + 1) for num in range(n - first + 1)]
        out += [(12, 0, 1, NULL), (0, 0, 0), (41, 0, 0), (41, 50, 0), (12, 13, 0), (12, 12, 1), (12, 0, 13), (12, 5, 8), (12, big, 0),
                (12, 0, big), (12, big, big), (40, 40, 1), (40, 0, 41)]
        return out
    if entry == "permutation":
        out = list(_range_cases(rng, 500, True))
        out += [(14, 0, 0, 3, 10), (14, 1, 1, 1, 11), (13, 1, 0, 1, 12), (12, 0, 0, 2, 10)]              # tiles that share lines
        out += [(12, 0, 0, 0, 1, NULL), (0, 0, 0, 0, 0), (41, 0, 0, 0, 0), (12, 1, 3, 4, 1), (12, 1, 3, 13, 1), (40, 0, 16, 0, 13),
                (12, 0, 0, 13, 0), (12, 0, 0, 12, 1), (12, 0, 0, 0, 13), (12, 0, 0, big, big), (12, 0, 0, big, 0), (12, 0, 0, 0, big),
                (12, (1 << 64) - 1, 0, 0, 0), (12, 1 << 12, 0, 0, 4), (12, 1 << 40, 1 << 40, 0, 4), (12, 16, 0, 4, 1), (12, 32, 32, 4, 2),
                (12, 1 << 12, 0, 4, 13), (40, 0, 0, 0, 13), (40, 0, 0, 27, 13), (40, 1 << 13, 0, 0, 13), (14, 0, 0, 0, 14)]
        return out
    out = list(_target_cases(rng, (1, 2, 3, 4, 5), 500))
    out += [(12, 0, 0, (0, 1, 2), NULL), (12, 0, 0, NO_TARGETS), (0, 0, 0, (0, 1, 2)), (41, 0, 0, (0, 1, 2)), (12, 1, 3, ()), (12, 0, 0, ()),
            (12, 1, 3, (0, 1, 2, 3, 4, 5)), (12, 8, 24, (4, 1, 4)), (12, 8, 24, (4, 1, 12)), (12, 0, 0, (4, 1, 4)), (12, 0, 0, (4, 4)),
            (2, 0, 0, (0, 1, 2)), (12, 0, 0, (12,)), (12, 0, 0, (0, big)), (12, (1 << 64) - 1, 0, (0, 1, 2)), (12, 1 << 12, 0, (0, 1, 2)),
            (12, 1, 1, (0, 1, 2)), (12, 4, 0, (0, 1, 2)), (40, 1 << 40, 0, (39,)), (12, 1, 3, (0, 0)), (12, 0, 0, (0, 1, 2, 3, 4, 5, 6))]
    return out


SENTINEL_ARGS = (40, 0, 0xDEAD, 0, 0)         # a qcx_permutation_plan call no case makes: refused with a text of its own


class Caller:
    """calls one entry point of the library of package `qc` and spells the answers"""

    def __init__(self, qc, entry):
        _lib = sys.modules[qc.__name__ + "._lib"]
        self.entry, self.lib = entry, qc.lib()
        self.plan = {"mc": _lib.McPlan, "diagonal": _lib.DiagPlan, "permutation": _lib.PermPlan, "multi": _lib.MultiPlan}[entry]()
        self.fn = getattr(self.lib, {"mc": "qcx_mc_gate_plan", "diagonal": "qcx_diagonal_plan", "permutation": "qcx_permutation_plan",
                                     "multi": "qcx_multi_gate_plan"}[entry])
        self.scrap = _lib.PermPlan()
        self.sentinel = None

    def plant(self):
        st = self.lib.qcx_permutation_plan(*SENTINEL_ARGS, C.byref(self.scrap))
        self.sentinel = self.lib.qcx_last_error()
        assert st == 2 and b"0xdead" in self.sentinel

    def line(self, args):
        """the canonical line of one call"""
        if self.sentinel is None:
            self.plant()
        null_out = args[-1] == NULL
        a = list(args[:-1] if null_out else args)
        head = f"{self.entry} " + " ".join(str(v) for v in args)
        if self.entry == "multi":
            t = a.pop()
            if t == NO_TARGETS:
                a += [0, None]
            else:
                a += [len(t), C.cast((C.c_uint * max(len(t), 1))(*t), C.c_void_p)]
        st = self.fn(*a, None if null_out else C.byref(self.plan))
        if st:
            err = self.lib.qcx_last_error()
            if err == self.sentinel:
                return f"{head} | refused {st}"
            self.sentinel = None
            return f"{head} | refused {st}: {err.decode()}"
        pl = self.plan
        vals = []
        for k in FIELDS[self.entry]:
            v = getattr(pl, k)
            vals.append(f"{k}={bytes(v).hex() if k in ARRAYS else v.decode() if k == 'kernel' else v}")
        return f"{head} | 0 | " + " ".join(vals)


def answer_lines(qc, entry):
    """every line of one entry point under the knobs of the moment"""
    c = Caller(qc, entry)
    return [c.line(a) for a in cases(entry)]


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def record(qc):
    """the golden file's content from the library of package `qc`"""
    old = {k: qc.lib().qcx_tune_get(k.encode()) for k in KNOBS}
    out = {"comment": "the answers of qcx_mc_gate_plan, qcx_diagonal_plan, qcx_permutation_plan and qcx_multi_gate_plan at commit 14ef617 "
                      "over tests/table_gate_plan_cases.py: one SHA-256 per entry point and knob set over the canonical lines joined by "
                      "newlines, the number of cases per entry point, and a readable sample of lines",
           "commit": "14ef617", "cases": {}, "digests": {}, "sample": []}
    for entry in ENTRIES:
        out["digests"][entry] = {}
        for name, knobs in KNOB_SETS[entry].items():
            qc.tune(**{k: knobs.get(k, v) for k, v in old.items()})
            lines = answer_lines(qc, entry)
            out["cases"][entry] = len(lines)
            out["digests"][entry][name] = digest(lines)
            rng = random.Random(f"sample {entry} {name}")
            ok = [ln for ln in lines if " | 0 | " in ln]
            bad = [ln for ln in lines if " | refused " in ln]
            out["sample"] += [{"entry": entry, "knobs": name, "line": ln} for ln in rng.sample(ok, 2) + rng.sample(bad, 1)]
    qc.tune(**old)
    return out


if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1])
    import quantumcomputer_amd
    assert quantumcomputer_amd.__file__.startswith(sys.argv[1])
    quantumcomputer_amd.lib()
    json.dump(record(quantumcomputer_amd), sys.stdout, indent=1)
    print()
