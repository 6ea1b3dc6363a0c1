"""CPU: qcx_multi_gate_plan (include/qcx_plan.h), the launch rule of qcx_mc_multi_qubit_gate on its own -- the library launches
from this very function.  K20's pass is emulated in numpy from the plan's fields alone (multi_qubit_ref.emulate): which amplitude
each (unit, element) stands for, which groups fire, which units are skipped, and the rows each group takes.  The indices computed
must be exactly the firing groups' members, each once; every tile must be closed under the target bits; and the emulated pass
must leave what tests/multi_qubit_ref.py defines.  The launch geometry is audited at widths no test allocates, the refusals in
their order, and qcx_permutation_plan -- which now shares its geometry code with this plan -- against its header's rule.
No GPU needed."""
import ctypes as C
import itertools

import numpy as np
import pytest

import multi_qubit_ref as mq
from bitwise import random_unitary, same

BAD_ARGUMENTS, BAD_QUBIT = 2, 6


def plan(qc, n, cm, cv, targets):
    st, pl = qc.multi_gate_plan(n, cm, cv, targets)
    assert st == 0, (n, cm, cv, targets, st, qc.lib().qcx_last_error())
    return pl


def check_fields(pl, n, cm, cv, targets):
    what = (n, hex(cm), hex(cv), targets)
    k = len(targets)
    squeezed = cm & ~7
    unsq = n - bin(squeezed).count("1")
    T = min(12, unsq)
    tm = sum(1 << q for q in targets)
    assert (pl.T, pl.num_targets) == (T, k) and list(pl.targets)[:k] == list(targets), what
    assert pl.squeezed == squeezed and pl.or_const == cv & squeezed, what
    tile, unit = int(pl.tile_mask), int(pl.unit_mask)
    assert bin(tile).count("1") == T and tile & tm == tm and tile & squeezed == 0 and tile & unit == 0, what
    assert tile | unit | squeezed == (1 << n) - 1 and unit & squeezed == 0, what
    others = [b for b in range(n) if not (squeezed >> b) & 1 and not (tm >> b) & 1]
    assert tile & ~tm == sum(1 << b for b in others[:T - k]), what               # the lowest other unsqueezed bits
    assert list(pl.tile_bits)[:T] == [b for b in range(n) if (tile >> b) & 1], what
    for j, q in enumerate(targets):
        assert pl.target_pos[j] == bin(tile & ((1 << q) - 1)).count("1") and pl.tile_bits[pl.target_pos[j]] == q, what
    runs = [(pl.run_pos[j], pl.run_len[j]) for j in range(pl.nruns)]
    assert sum(((1 << l) - 1) << p for p, l in runs) == squeezed and all(runs[j][0] + runs[j][1] < runs[j + 1][0] for j in range(len(runs) - 1)), what
    low = cm & 7
    assert pl.elem_mask == low and pl.elem_values == cv & low, what              # bits 0-2 always lie inside the tile ...
    assert pl.unit_mask_low == 0 and pl.unit_values_low == 0 and pl.form == 0, what      # ... so no tile predicate, whole lines
    assert tile & 7 == 7 & ((1 << n) - 1), what
    assert pl.units == 1 << (unsq - T), what
    assert pl.rows_per_item == (2 if k == 1 else 4), what
    assert pl.block == min(1024, max(64, (1 << T) // pl.rows_per_item)) and 1 <= pl.grid <= pl.units, what
    assert pl.block * (2 if k == 1 else 1) * pl.rows_per_item >= 1 << T, what    # every row of every group has its work item
    assert pl.lds_bytes == 16 << T and pl.lds_bytes <= 65536, what
    assert pl.store_all == (1 if low else 0), what
    assert pl.kernel.decode() == "k_multi_tile<%d, %s>" % (k, "true" if pl.nt else "false"), what


def check(qc, n, cm, cv, targets, seed):
    pl = plan(qc, n, cm, cv, targets)
    check_fields(pl, n, cm, cv, targets)
    what = (n, hex(cm), hex(cv), targets)
    U = random_unitary(seed, 1 << len(targets))
    rs = np.random.RandomState(seed)
    state = rs.standard_normal(2 << n)
    got, computed, read, skipped = mq.emulate(pl, U, state, n, targets)
    idx = np.arange(1 << n, dtype=np.uint64)
    firing = idx[(idx & np.uint64(cm)) == np.uint64(cv)]
    assert np.array_equal(computed, firing), what                               # exactly the firing groups' members, each once
    assert skipped == 0 and read == int(pl.units), what                          # (no tile predicate exists: see check_fields)
    # every tile is closed under the target bits: flipping any target bit of a tile's index stays in the tile
    tm = sum(1 << q for q in targets)
    assert int(pl.tile_mask) & tm == tm and int(pl.unit_mask) & tm == 0 and int(pl.squeezed) & tm == 0, what
    want = mq.apply(state, n, targets, U, cm, cv)
    keep = np.ones(1 << n, dtype=bool); keep[firing.astype(np.int64)] = False
    w = want.reshape(-1, 2).copy(); w[keep] = state.reshape(-1, 2)[keep]        # (a finite pass leaves the others as they are)
    same(got, w.reshape(-1), what)
    return pl


@pytest.mark.parametrize("n", list(range(3, 15)))
def test_the_pass_of_small_registers(qc, n):
    count = 60 if n <= 10 else 24
    ks = set()
    for j, (targets, cm, cv) in enumerate(mq.draws(n, count, 1000 + n)):
        ks.add(len(targets))
        check(qc, n, cm, cv, targets, 31 * n + j)
    assert ks == set(range(1, min(5, n) + 1))


def test_the_draws_cover_their_strata():
    d = mq.draws(14, 400, 5)
    cls = lambda q: 0 if q < 3 else 1 if q < 6 else 2
    assert {len(t) for t, _, _ in d} == {1, 2, 3, 4, 5}
    assert {cls(q) for t, _, _ in d for q in t} == {0, 1, 2}
    assert any(all(q < 3 for q in t) for t, _, _ in d if len(t) == 3) and any(all(q >= 6 for q in t) for t, _, _ in d if len(t) == 5)
    assert any(list(t) != sorted(t) for t, _, _ in d)
    assert any(m and not m & ~7 for _, m, _ in d) and any(m and not m & 7 for _, m, _ in d) and any(m & 7 and m & ~7 for _, m, _ in d)
    assert any(m and v == m for _, m, v in d) and any(m and v == 0 for _, m, v in d) and any(m and 0 < v < m and v != m for _, m, v in d)
    assert any(bin(m).count("1") == 14 - len(t) for t, m, _ in d) and any(m == 0 for _, m, _ in d)


def test_every_form_of_n5_with_three_targets(qc):
    """every ordered triple of n = 5 under every mask and polarity of the other two qubits"""
    j = 0
    for t in itertools.permutations(range(5), 3):
        free = [q for q in range(5) if q not in t]
        for cs in ([], [free[0]], [free[1]], free):
            cm = sum(1 << c for c in cs)
            for pol in range(1 << len(cs)):
                cv = sum(1 << c for b, c in enumerate(cs) if (pol >> b) & 1)
                check(qc, 5, cm, cv, t, j)
                j += 1


@pytest.mark.parametrize("knob,value", [("multi_grid_cap", 3), ("multi_grid_cap", 0), ("multi_store_all", 0), ("multi_nt", 1)])
def test_knobs(qc, knob, value):
    keep = qc.lib().qcx_tune_get(knob.encode())
    qc.tune(**{knob: value})
    try:
        for n, cm, cv, t in [(14, 0, 0, (2, 9, 13)), (14, 1, 1, (3, 4, 5, 6)), (14, 0x2002, 0x2000, (4, 0, 8, 2, 11)), (13, 4, 0, (0, 1))]:
            st, pl = qc.multi_gate_plan(n, cm, cv, t)
            assert st == 0
            if knob == "multi_grid_cap":
                assert pl.grid == (min(int(pl.units), value) if value else int(pl.units))
            elif knob == "multi_store_all":
                assert pl.store_all == 0
            else:
                assert pl.nt == 1 and pl.kernel.decode().endswith(", true>")
    finally:
        qc.tune(**{knob: keep})
    pl = plan(qc, 14, 1, 1, (3, 4, 5, 6))
    assert (pl.store_all, pl.nt, pl.T) == (1, 0, 12) and pl.grid == min(int(pl.units), 2048) and plan(qc, 14, 8, 8, (4, 5, 6)).store_all == 0


def test_geometry_of_wide_registers(qc):
    for n in (30, 32, 33, 34, 40):
        for t in [(0, 1, 2), (3, 4, 5), (n - 3, n - 2, n - 1), (n - 1, 0, 13), (3, 14, 22, 29), (2, 9, 14, 22, 29), (n - 1, n - 2, n - 3, n - 4, n - 5), (7,), (n - 1, 4)]:
            for cs in ([], [n - 1], [3], [0], [n - 1, n - 2, 5], [31, 32] if n > 32 else [20, 21], list(range(3, n, 2))):
                cs = [c for c in cs if c not in t and c < n]
                cm = sum(1 << c for c in cs)
                cv = sum(1 << c for c in cs[::2])
                pl = plan(qc, n, cm, cv, t)
                check_fields(pl, n, cm, cv, t)
                sq = bin(cm & ~7).count("1")
                assert pl.units << pl.T == 1 << (n - sq) and pl.T == min(12, n - sq)      # counts beyond 2^32 at n = 33, 34
                assert pl.grid == min(int(pl.units), 2048)
                # the last element of the last unit is the highest index that fires on the squeezed controls
                last = int(mq.deposit(np.array([(1 << (n - sq - pl.T)) - 1], dtype=np.uint64), pl.unit_mask)[0]) | int(pl.tile_mask) | int(pl.or_const)
                assert last == ((1 << n) - 1) & ~((cm & ~7) & ~cv)
    keep = qc.lib().qcx_tune_get(b"multi_grid_cap")
    qc.tune(multi_grid_cap=0)
    try:
        assert plan(qc, 33, 0, 0, (0, 1, 2)).grid == 1 << 21 and plan(qc, 34, 0, 0, (5, 6, 7)).grid == 0xFFFFFFFF // 1024      # HIP: grid * block < 2^32
    finally:
        qc.tune(multi_grid_cap=keep)


def test_refusals_in_their_order(qc):
    L = qc.lib()
    pl = qc._lib.MultiPlan()
    p = C.byref(pl)
    arr = lambda *t: C.cast((C.c_uint * max(len(t), 1))(*t), C.c_void_p)
    assert L.qcx_multi_gate_plan(0, 0, 0, 1, arr(0), p) == BAD_ARGUMENTS
    assert L.qcx_multi_gate_plan(41, 0, 0, 1, arr(0), p) == BAD_ARGUMENTS
    assert L.qcx_multi_gate_plan(12, 0, 0, 1, arr(0), None) == BAD_ARGUMENTS
    assert L.qcx_multi_gate_plan(12, 0, 0, 1, None, p) == BAD_ARGUMENTS
    assert L.qcx_multi_gate_plan(40, 0, 0, 5, arr(39, 0, 20, 3, 38), p) == 0
    for k in (0, 6, 0xFFFFFFFF):
        assert L.qcx_multi_gate_plan(12, 0x10, 0x30, k, arr(0, 0, 99, 1, 2, 3), p) == BAD_ARGUMENTS      # the count before everything else
        assert b"1 to 5" in L.qcx_last_error()
    assert L.qcx_multi_gate_plan(12, 0x10, 0x30, 3, arr(0, 0, 99), p) == BAD_ARGUMENTS                   # values outside the mask before the targets
    assert b"ctrl_values 0x30 has bits outside ctrl_mask 0x10" in L.qcx_last_error()
    for n, t in [(5, (5, 0, 1)), (5, (0, 1, 0xFFFFFFFF)), (12, (3, 4, 3)), (12, (1, 1)), (3, (0, 1, 2, 3)), (12, (64, 1, 2))]:
        assert L.qcx_multi_gate_plan(n, 0, 0, len(t), arr(*t), p) == BAD_QUBIT, (n, t)
    for n, cm, t in [(12, 1 << 12, (0, 1, 2)), (12, 1 << 63, (0, 1, 2)), (12, 1 << 3, (2, 3, 4)), (40, 1 << 40, (0, 1, 2)), (12, 0xFFF, (5, 6, 7))]:
        assert L.qcx_multi_gate_plan(n, cm, 0, len(t), arr(*t), p) == BAD_QUBIT, (n, cm, t)
    assert qc.multi_qubit_max_targets() == 5


def test_permutation_plan_is_unchanged(qc):
    """qcx_permutation_plan's fields, recomputed here from the rule in its header comment (include/qcx_plan.h), for a sample
    that covers no control, squeezed and low controls, small registers, shared lines and the tile predicate"""
    sample = [(14, 0, 0, 2, 9), (14, 1, 1, 3, 9), (14, 0x2002, 0x2000, 4, 3), (13, 4, 0, 0, 2), (7, 1, 0, 2, 2), (14, 1, 0, 2, 12), (13, 0, 0, 1, 10),
              (30, (1 << 29) | (1 << 11) | 2, 1 << 11, 12, 8), (33, (1 << 32) | (1 << 31), 1 << 32, 3, 4), (5, 0, 0, 0, 5), (1, 0, 0, 0, 0), (40, 5, 4, 28, 12)]
    for n, cm, cv, first, num in sample:
        st, pl = qc.permutation_plan(n, cm, cv, first, num)
        what = (n, hex(cm), hex(cv), first, num)
        assert st == 0, what
        squeezed = cm & ~7
        unsq = n - bin(squeezed).count("1")
        T = min(12, unsq, max(num + 3, 12))
        rng = ((1 << num) - 1) << first
        others = [b for b in range(n) if not (squeezed >> b) & 1 and not (rng >> b) & 1]
        tile = rng | sum(1 << b for b in others[:T - num])
        unit = sum(1 << b for b in others[T - num:])
        assert (pl.T, pl.first, pl.num, int(pl.tile_mask), int(pl.unit_mask)) == (T, first, num, tile, unit), what
        assert list(pl.tile_bits)[:T] == [b for b in range(n) if (tile >> b) & 1] and not any(list(pl.tile_bits)[T:]), what
        assert pl.range_pos == bin(tile & ((1 << first) - 1)).count("1"), what
        assert (int(pl.squeezed), int(pl.or_const)) == (squeezed, cv & squeezed), what
        runs, b = [], 0
        while b < n:
            if (squeezed >> b) & 1:
                ln = 1
                while b + ln < n and (squeezed >> (b + ln)) & 1:
                    ln += 1
                runs.append((b, ln)); b += ln
            else:
                b += 1
        assert [(pl.run_pos[j], pl.run_len[j]) for j in range(pl.nruns)] == runs, what
        low = cm & 7
        assert (pl.elem_mask, pl.elem_values, pl.unit_mask_low, pl.unit_values_low) == (low & tile, cv & low & tile, low & ~tile, cv & low & ~tile), what
        assert pl.units == 1 << (unsq - T) and pl.block == (1024 if T == 12 else 256) and pl.grid == min(int(pl.units), 2048), what
        assert pl.lds_bytes == (16 << T) + ((2 << num) + 15) // 16 * 16, what
        assert pl.form == (0 if tile & 7 == 7 & ((1 << n) - 1) else 1) and pl.store_all == (1 if low else 0) and pl.nt == 0, what
        assert pl.kernel.decode() == "k_perm_tile<false, false>", what
    assert {qc.permutation_plan(*s)[1].form for s in sample} == {0, 1} and any(qc.permutation_plan(*s)[1].unit_mask_low for s in sample)


KNOB_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.qcx_tune_get.restype = ctypes.c_long
lib.qcx_tune_get.argtypes = [ctypes.c_char_p]
lib.qcx_tune_set.argtypes = [ctypes.c_char_p, ctypes.c_long]
names = [b"multi_grid_cap", b"multi_store_all", b"multi_nt", b"multi_generic", b"perm_nt", b"mc_generic"]
defaults = [lib.qcx_tune_get(k) for k in names]
for i, k in enumerate(names):
    assert lib.qcx_tune_set(k, 700 + i) == 0, k
print(json.dumps({"defaults": defaults, "back": [lib.qcx_tune_get(k) for k in names]}))
"""


def test_the_knobs_defaults_in_a_fresh_process(qc):
    """multi_grid_cap = 2048, multi_store_all = 1, multi_nt = 0, multi_generic = 0, and the neighbours they were added between
    keep theirs; a value set is the value read back and aliases no neighbour (a child process that never touches a device)"""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", KNOB_CHILD, qc.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got == {"defaults": [2048, 1, 0, 0, 0, 0], "back": [700, 701, 702, 703, 704, 705]}


def test_matrix_permutation_checks_and_plan_under_host_sanitizers(tmp_path):
    """tests/c/multi_gate_sanitize.cpp: the library's source around a main of its own, host side built under AddressSanitizer
    and UBSan (device code built normally), run over a grid of target sets and controls, hostile knobs, the refusals and the
    host-side matrix permutation (CPU only, its own process)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "multi_gate_sanitize")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    host_only = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]      # the host side alone
    subprocess.run([hipcc, "-O1", "-g", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", *host_only, "-o", exe,
                    os.path.join(root, "tests", "c", "multi_gate_sanitize.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "multi_gate_sanitize ok" in r.stdout, r.stdout + r.stderr
