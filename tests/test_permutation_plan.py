"""CPU: qcx_permutation_plan (include/qcx_plan.h), the launch rule of qcx_permutation_gate on its own -- the library launches from
this very function.  K19's walk is emulated in numpy from the plan's fields alone: which amplitude each (unit, element) stands
for, which of them fire, which units are skipped, and where an element takes its source from.  The indices visited must be
exactly the firing set, each once; every tile must be closed under the table; and the emulated pass must leave what
tests/permutation_ref.py defines.  Its launch geometry is audited at widths no test allocates.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import permutation_ref as pr

BAD_ARGUMENTS, BAD_QUBIT = 2, 6


def plan(qc, n, cm, cv, first, num):
    st, pl = qc.permutation_plan(n, cm, cv, first, num)
    assert st == 0, (n, cm, cv, first, num, st)
    return pl


def control_sets(n, first, num):
    """no control; one control at bits 0, 2, 3, first - 1, first + num and n - 1, in both polarities; two and three mixed ones"""
    free = [c for c in sorted({0, 2, 3, first - 1, first + num, n - 1}) if 0 <= c < n and not first <= c < first + num]
    out = [(0, 0)]
    for c in free:
        out += [(1 << c, 1 << c), (1 << c, 0)]
    if len(free) >= 2:
        out.append(((1 << free[0]) | (1 << free[-1]), 1 << free[0]))
        out.append(((1 << free[0]) | (1 << free[-1]), 1 << free[-1]))
    if len(free) >= 3:
        out.append(((1 << free[0]) | (1 << free[1]) | (1 << free[-1]), (1 << free[1])))
    return out


def check_fields(pl, n, cm, cv, first, num, tile_log2=12):
    what = (n, hex(cm), hex(cv), first, num)
    squeezed = cm & ~7
    unsq = n - bin(squeezed).count("1")
    T = min(12, unsq, max(num + 3, tile_log2))                               # the default: min(12, unsq)
    rng = ((1 << num) - 1) << first
    assert (pl.T, pl.first, pl.num) == (T, first, num) and pl.squeezed == squeezed and pl.or_const == cv & squeezed, what
    tile, unit = int(pl.tile_mask), int(pl.unit_mask)
    assert bin(tile).count("1") == T and tile & rng == rng and tile & squeezed == 0 and tile & unit == 0, what
    assert tile | unit | squeezed == (1 << n) - 1 and unit & squeezed == 0, what
    others = [b for b in range(n) if not (squeezed >> b) & 1 and not (rng >> b) & 1]
    assert tile & ~rng == sum(1 << b for b in others[:T - num]), what        # the lowest other unsqueezed bits
    assert list(pl.tile_bits)[:T] == [b for b in range(n) if (tile >> b) & 1], what
    assert pl.range_pos == bin(tile & ((1 << first) - 1)).count("1"), what
    runs = [(pl.run_pos[k], pl.run_len[k]) for k in range(pl.nruns)]
    assert sum(((1 << l) - 1) << p for p, l in runs) == squeezed and all(runs[k][0] + runs[k][1] < runs[k + 1][0] for k in range(len(runs) - 1)), what
    low = cm & 7
    assert pl.elem_mask == low & tile and pl.elem_values == cv & low & tile, what
    assert pl.unit_mask_low == low & ~tile and pl.unit_values_low == cv & low & ~tile, what
    assert pl.units == 1 << (unsq - T) and pl.units << T == 1 << (n - bin(squeezed).count("1")), what
    assert pl.block == (1024 if T == 12 else 256) and 1 <= pl.grid <= pl.units, what
    assert pl.lds_bytes == (16 << T) + ((2 << num) + 15) // 16 * 16 and pl.lds_bytes <= 73728, what
    whole = tile & 7 == 7 & ((1 << n) - 1)
    assert pl.form == (0 if whole else 1), what
    if num <= 9:
        assert whole, what                                                   # whole 128-B lines as long as num <= 9
    assert pl.kernel.decode() == "k_perm_tile<false, %s>" % ("true" if pl.nt else "false"), what


def walk(pl, n, perm):
    """the pass, emulated: returns (new, visited) where new[i] = the index whose amplitude lands on i (i itself where nothing is
    stored) and visited = every index an element that fires stands for, in walk order"""
    T, pf, num = int(pl.T), int(pl.range_pos), int(pl.num)
    inv = pr.inverse(perm, num)
    e = np.arange(1 << T, dtype=np.int64)
    off = pr.deposit(e, pl.tile_mask)
    src_e = (e & ~(((1 << num) - 1) << pf)) | (inv[(e >> pf) & ((1 << num) - 1)] << pf)
    acts = (off & pl.elem_mask) == pl.elem_values
    new = np.arange(1 << n, dtype=np.int64)
    visited, skipped = [], []
    base = pr.deposit(np.arange(int(pl.units), dtype=np.int64), pl.unit_mask) | int(pl.or_const)
    for b in base.tolist():
        if (b & pl.unit_mask_low) != pl.unit_values_low:
            skipped.append(b)
            continue
        i = b | off
        assert int(i.max()) < 1 << n
        tile_set = set(i.tolist())
        assert set((b | off[src_e]).tolist()) == tile_set                    # closed under the table: every source is in the tile
        new[i[acts]] = (b | off[src_e])[acts]
        visited.append(i[acts])
    return new, (np.concatenate(visited) if visited else np.zeros(0, np.int64)), skipped


def check(qc, n, cm, cv, first, num, rs, tile_log2=12):
    pl = plan(qc, n, cm, cv, first, num)
    check_fields(pl, n, cm, cv, first, num, tile_log2)
    perm = rs.permutation(1 << num)
    new, visited, skipped = walk(pl, n, perm)
    what = (n, hex(cm), hex(cv), first, num)
    firing = np.flatnonzero(pr.fires(n, cm, cv))
    assert np.array_equal(np.sort(visited), firing), what                    # exactly the firing set, each once
    assert np.array_equal(new, pr.source(n, first, num, perm, cm, cv)), what
    # the skipped units are exactly those whose low controls miss: none of their indices fires
    low_outside = pl.unit_mask_low
    for b in skipped:
        assert (b & low_outside) != (cv & low_outside), what
    if not low_outside:
        assert not skipped, what
    else:
        assert len(skipped) == int(pl.units) - (int(pl.units) >> bin(low_outside).count("1")), what
    return pl


@pytest.mark.parametrize("n", list(range(1, 15)))
def test_the_walk_of_small_registers(qc, n):
    rs = np.random.RandomState(n)
    forms = set()
    for first in range(n + 1):
        nums = range(min(12, n - first) + 1)
        if n > 10:
            nums = sorted({k for k in (0, 1, 4, 9, 10, 11, 12, n - first) if k <= min(12, n - first)})
        for num in nums:
            for cm, cv in control_sets(n, first, num):
                forms.add(check(qc, n, cm, cv, first, num, rs).form)
    assert forms == ({0, 1} if n >= 13 else {0})                             # shared lines: num >= 10, first > 0 and more than one tile


@pytest.mark.parametrize("knob,value", [("perm_grid_cap", 3), ("perm_grid_cap", 0), ("perm_store_all", 0), ("perm_nt", 1), ("perm_tile_log2", 8),
                                        ("perm_tile_log2", 10), ("perm_tile_log2", 0), ("perm_tile_log2", 99)])
def test_knobs(qc, knob, value):
    keep = qc.lib().qcx_tune_get(knob.encode())
    qc.tune(**{knob: value})
    rs = np.random.RandomState(3)
    try:
        for n, cm, cv, first, num in [(14, 0, 0, 2, 9), (14, 1, 1, 3, 9), (14, 0x2002, 0x2000, 4, 3), (13, 4, 0, 0, 2), (7, 1, 0, 2, 2)]:
            pl = check(qc, n, cm, cv, first, num, rs, min(12, value) if knob == "perm_tile_log2" else 12)
            if knob == "perm_tile_log2":
                assert pl.T == min(12, n - bin(cm & ~7).count("1"), max(num + 3, min(12, value)))
            elif knob == "perm_grid_cap":
                assert pl.grid == (min(int(pl.units), value) if value else int(pl.units))
            elif knob == "perm_store_all":
                assert pl.store_all == 0
            else:
                assert pl.nt == 1
    finally:
        qc.tune(**{knob: keep})
    pl = plan(qc, 14, 1, 1, 3, 9)
    assert (pl.store_all, pl.nt, pl.T) == (1, 0, 12) and pl.grid == min(int(pl.units), 2048) and plan(qc, 14, 8, 8, 4, 9).store_all == 0


def test_geometry_of_wide_registers(qc):
    for n in (30, 32, 33, 34, 40):
        for first, num in [(0, 0), (0, 5), (0, 12), (3, 9), (8, 4), (12, 8), (18, 12), (n - 4, 4), (n - 12, 12), (29, 4), (n, 0), (1, 12)]:
            if first + num > n:
                continue
            for cs in ([], [n - 1], [3], [0], [n - 1, n - 2, 5], [31, 32] if n > 32 else [20, 21], list(range(3, n, 2))):
                cs = [c for c in cs if not first <= c < first + num and c < n]
                cm = sum(1 << c for c in cs)
                cv = sum(1 << c for c in cs[::2])
                pl = plan(qc, n, cm, cv, first, num)
                check_fields(pl, n, cm, cv, first, num)
                sq = bin(cm & ~7).count("1")
                assert pl.units << pl.T == 1 << (n - sq) and pl.T == min(12, n - sq)      # counts beyond 2^32 at n = 33, 34
                assert pl.or_const == cv & ~7 and pl.grid == min(int(pl.units), 2048)
                # the last element of the last unit is the highest index that fires on the squeezed controls
                last = int(pr.deposit((1 << (n - sq - pl.T)) - 1, pl.unit_mask)) | int(pr.deposit((1 << pl.T) - 1, pl.tile_mask)) | int(pl.or_const)
                assert last == ((1 << n) - 1) & ~((cm & ~7) & ~cv)
    keep = qc.lib().qcx_tune_get(b"perm_grid_cap")
    qc.tune(perm_grid_cap=0)
    try:
        assert plan(qc, 33, 0, 0, 0, 9).grid == 1 << 21 and plan(qc, 34, 0, 0, 0, 9).grid == 0xFFFFFFFF // 1024      # HIP: grid * block < 2^32
    finally:
        qc.tune(perm_grid_cap=keep)


def test_refusals(qc):
    L = qc.lib()
    pl = qc._lib.PermPlan()
    p = C.byref(pl)
    assert L.qcx_permutation_plan(0, 0, 0, 0, 0, p) == BAD_ARGUMENTS
    assert L.qcx_permutation_plan(41, 0, 0, 0, 1, p) == BAD_ARGUMENTS
    assert L.qcx_permutation_plan(12, 0, 0, 0, 1, None) == BAD_ARGUMENTS
    assert L.qcx_permutation_plan(40, 0, 0, 28, 12, p) == 0
    assert L.qcx_permutation_plan(12, 0x10, 0x30, 0, 1, p) == BAD_ARGUMENTS                     # values outside the mask ...
    assert b"ctrl_values 0x30 has bits outside ctrl_mask 0x10" in L.qcx_last_error()
    assert L.qcx_permutation_plan(12, 0x10, 0x30, 12, 1, p) == BAD_ARGUMENTS                    # ... before the range
    for n, first, num in [(5, 0, 6), (5, 5, 1), (5, 6, 0), (12, 11, 2), (30, 0xFFFFFFFF, 1), (30, 1, 0xFFFFFFFF), (30, 0xFFFFFFFF, 0xFFFFFFFF), (30, 10, 21)]:
        assert L.qcx_permutation_plan(n, 0, 0, first, num, p) == BAD_QUBIT, (n, first, num)     # (a range past n before its width)
    for n, cm, first, num in [(12, 1 << 12, 0, 1), (12, 1 << 63, 0, 1), (12, 1 << 3, 3, 1), (12, 1 << 5, 2, 4), (40, 1 << 40, 0, 1), (30, 1 << 20, 10, 13)]:
        assert L.qcx_permutation_plan(n, cm, 0, first, num, p) == BAD_QUBIT, (n, cm, first, num)    # (a control in the range before its width)
    for n, first, num in [(13, 0, 13), (30, 10, 13), (40, 0, 40)]:
        assert L.qcx_permutation_plan(n, 0, 0, first, num, p) == BAD_ARGUMENTS, (n, first, num)
        assert b"12" in L.qcx_last_error()
    assert qc.permutation_max_qubits() == 12


KNOB_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.qcx_tune_get.restype = ctypes.c_long
lib.qcx_tune_get.argtypes = [ctypes.c_char_p]
lib.qcx_tune_set.argtypes = [ctypes.c_char_p, ctypes.c_long]
names = [b"perm_grid_cap", b"perm_store_all", b"perm_nt", b"perm_tile_log2"]
defaults = [lib.qcx_tune_get(k) for k in names]
for i, k in enumerate(names):
    assert lib.qcx_tune_set(k, 700 + i) == 0, k
print(json.dumps({"defaults": defaults, "back": [lib.qcx_tune_get(k) for k in names]}))
"""


def test_the_knobs_defaults_in_a_fresh_process(qc):
    """perm_grid_cap = 2048, perm_store_all = 0, perm_nt = 0, perm_tile_log2 = 12; a value set is the value read back and aliases no neighbour (a child
    process that never touches a device: this one's knobs may have been turned by other tests)"""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", KNOB_CHILD, qc.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got == {"defaults": [2048, 1, 0, 12], "back": [700, 701, 702, 703]}


def test_table_check_and_plan_under_host_sanitizers(tmp_path):
    """tests/c/permutation_sanitize.cpp: the library's source around a main of its own, host side built under AddressSanitizer
    and UBSan (device code built normally), run over this file's grid, the strict form, hostile knobs and malformed tables (CPU
    only, its own process)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "permutation_sanitize")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    host_only = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]      # the host side alone
    subprocess.run([hipcc, "-O1", "-g", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", *host_only, "-o", exe,
                    os.path.join(root, "tests", "c", "permutation_sanitize.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "permutation_sanitize ok" in r.stdout, r.stdout + r.stderr
