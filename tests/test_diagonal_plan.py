"""CPU: qcx_diagonal_plan (include/qcx_plan.h), the launch rule of qcx_diagonal_gate on its own -- the library launches from this
very function.  K18's walk is emulated in numpy from the plan's fields alone: which amplitude each (unit, thread, element)
touches and which table entry it takes.  Every index must turn up exactly once, with the definition's entry
(diagonal_ref.entry_index).  Its launch geometry is audited at widths no test allocates.  No GPU needed."""
import numpy as np
import pytest

import diagonal_ref as dr

BAD_ARGUMENTS, BAD_QUBIT = 2, 6


def plan(qc, n, first, num):
    st, pl = qc.diagonal_plan(n, first, num)
    assert st == 0, (n, first, num, st)
    return pl


def walk(pl):
    """(index, entry, workgroup) of every element the launch touches, in the kernel's terms: workgroup b takes the units
    b, b + grid, ...; thread tid owns e = tid + 256 j, j < elems, where e < 2^T; i = (u << T) | e; and the entry comes from where
    the form says it does"""
    T, first, kmask = int(pl.T), int(pl.first), int(pl.kmask)
    units = int(pl.units)
    u = np.arange(units, dtype=np.uint64)
    wg = (u % np.uint64(pl.grid)).astype(np.int64)
    # (the stride loop of workgroup b reaches exactly the units congruent to b; every b < grid exists)
    assert pl.grid >= 1 and (units < pl.grid or set(wg.tolist()) == set(range(pl.grid)))
    tid = np.arange(256, dtype=np.uint64)
    j = np.arange(int(pl.elems), dtype=np.uint64)
    e = (tid[None, :] + np.uint64(256) * j[:, None])                       # [j, tid]
    exists = e < np.uint64(1 << T)
    U, J, TID = np.meshgrid(u, j, tid, indexing="ij")
    E = TID + np.uint64(256) * J
    ok = E < np.uint64(1 << T)
    base = U << np.uint64(T)
    i = base | E
    if pl.form == 0:                                                        # QCX_DIAG_TILE: from the unit alone
        k = (base >> np.uint64(first)) & np.uint64(kmask)
    elif pl.form == 1:                                                      # QCX_DIAG_GROUP: from the unit and j
        k = ((base | (np.uint64(256) * J)) >> np.uint64(first)) & np.uint64(kmask)
    elif pl.lds:                                                            # QCX_DIAG_LANE out of LDS: from the element alone
        k = (E >> np.uint64(first)) & np.uint64(kmask)
        assert int(k[ok].max()) * 16 + 16 <= pl.lds_bytes
    else:
        k = (i >> np.uint64(first)) & np.uint64(kmask)
    assert not pl.full or (pl.elems == 16 and bool(exists.all()))          # full: nothing in the walk is guarded
    return i[ok], k[ok].astype(np.int64), np.broadcast_to(wg[:, None, None], i.shape)[ok]


def check(qc, n, first, num):
    pl = plan(qc, n, first, num)
    what = (n, first, num, pl.kernel)
    T = min(n, 12)
    assert (pl.T, pl.first, pl.num, pl.block) == (T, first, num, 256) and pl.kmask == (1 << num) - 1 and pl.units == 1 << (n - T), what
    assert pl.elems == (1 << (T - 8) if T > 8 else 1) and pl.full == (1 if T == 12 else 0), what
    want_form = 0 if (num == 0 or first >= T) else (1 if first >= 8 else 2)
    assert pl.form == want_form, what
    assert pl.kernel.decode() == "k_diagonal<%d, %s, %s>" % (pl.form, "true" if pl.full else "false", "true" if pl.lds else "false"), what
    assert pl.lds_bytes == (16 << num if pl.lds else 0) and pl.lds_bytes <= 65536, what
    if pl.lds:
        assert pl.form == 2 and first + num <= 12, what
    i, k, wg = walk(pl)
    order = np.argsort(i, kind="stable")
    assert np.array_equal(i[order], np.arange(1 << n, dtype=np.uint64)), what          # each index exactly once
    assert np.array_equal(k[order], dr.entry_index(n, first, num)), what
    # the entries one tile takes: slice_entries of them
    per_tile = 1 if pl.form == 0 else 1 << (min(first + num, T) - first)
    assert pl.slice_entries == per_tile, what
    tile0 = k[(i >> np.uint64(T)) == 0]
    assert np.unique(tile0).size == per_tile, what
    return pl


@pytest.mark.parametrize("n", list(range(1, 17)))
def test_every_range_of_small_registers(qc, n):
    forms = set()
    for first in range(n + 1):
        for num in range(n - first + 1):
            pl = check(qc, n, first, num)
            forms.add(pl.form)
            assert pl.grid == min(int(pl.units), 2048)
    assert forms == ({0, 1, 2} if n >= 9 else {0, 2})


@pytest.mark.parametrize("knob,value", [("diag_grid_cap", 3), ("diag_grid_cap", 5), ("diag_grid_cap", 0), ("diag_lds", 1)])
def test_knobs(qc, knob, value):
    keep = qc.lib().qcx_tune_get(knob.encode())
    qc.tune(**{knob: value})
    try:
        for n in (7, 12, 13, 15, 16):
            for first in range(n + 1):
                for num in sorted({min(k, n - first) for k in (0, 1, 4, n)}):
                    pl = check(qc, n, first, num)
                    if knob == "diag_grid_cap":
                        assert pl.grid == (min(int(pl.units), value) if value else int(pl.units))
                    else:
                        assert pl.lds == (1 if pl.form == 2 and first + num <= 12 else 0)
    finally:
        qc.tune(**{knob: keep})
    assert plan(qc, 16, 0, 4).lds == 0, "the default reads the table from memory"


def test_geometry_of_wide_registers(qc):
    for n in (30, 32, 33, 34, 40):
        for first, num in [(0, 0), (0, 1), (0, 12), (0, n), (5, 7), (8, 4), (10, 10), (12, 4), (n - 1, 1), (n, 0), (3, n - 3)]:
            pl = plan(qc, n, first, num)
            assert pl.units == 1 << (n - 12) and pl.kmask == (1 << num) - 1 and pl.grid == 2048 and pl.block == 256 and pl.full == 1
            assert pl.units * 4096 == 1 << n                                # counts beyond 2^32 at n = 33, 34
            # the highest element of the last unit is the register's last amplitude, and its entry the definition's
            i_last = ((int(pl.units) - 1) << 12) | (255 + 256 * (pl.elems - 1))
            assert i_last == (1 << n) - 1 and (i_last >> first) & int(pl.kmask) == (1 << num) - 1
            assert pl.lds == 0 and pl.lds_bytes == 0
    keep = qc.lib().qcx_tune_get(b"diag_grid_cap")
    qc.tune(diag_grid_cap=0)
    try:
        assert plan(qc, 34, 0, 34).grid == 1 << 22 and plan(qc, 40, 0, 1).grid == 0xFFFFFFFF // 256     # HIP: grid * block < 2^32
    finally:
        qc.tune(diag_grid_cap=keep)


def test_refusals(qc):
    L = qc.lib()
    pl = qc._lib.DiagPlan()
    import ctypes as C
    assert L.qcx_diagonal_plan(0, 0, 0, C.byref(pl)) == BAD_ARGUMENTS
    assert L.qcx_diagonal_plan(41, 0, 1, C.byref(pl)) == BAD_ARGUMENTS
    assert L.qcx_diagonal_plan(12, 0, 1, None) == BAD_ARGUMENTS
    assert L.qcx_diagonal_plan(40, 0, 40, C.byref(pl)) == 0
    for n, first, num in [(5, 0, 6), (5, 5, 1), (5, 6, 0), (12, 11, 2), (30, 0xFFFFFFFF, 1), (30, 1, 0xFFFFFFFF), (30, 0xFFFFFFFF, 0xFFFFFFFF)]:
        assert L.qcx_diagonal_plan(n, first, num, C.byref(pl)) == BAD_QUBIT, (n, first, num)


def test_host_maximum(qc):
    assert qc.diagonal_host_max_qubits() == 20


KNOB_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.qcx_tune_get.restype = ctypes.c_long
lib.qcx_tune_get.argtypes = [ctypes.c_char_p]
lib.qcx_tune_set.argtypes = [ctypes.c_char_p, ctypes.c_long]
names = [b"diag_grid_cap", b"diag_lds", b"prot_grid_cap"]
defaults = [lib.qcx_tune_get(k) for k in names]
for i, k in enumerate(names):
    assert lib.qcx_tune_set(k, 700 + i) == 0, k
print(json.dumps({"defaults": defaults, "back": [lib.qcx_tune_get(k) for k in names]}))
"""


def test_the_knobs_defaults_in_a_fresh_process(qc):
    """diag_grid_cap = 2048 like prot_grid_cap, diag_lds = 0; a value set is the value read back and aliases no neighbour (a
    child process that never touches a device: this one's knobs may have been turned by other tests)"""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", KNOB_CHILD, qc.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got == {"defaults": [2048, 0, 2048], "back": [700, 701, 702]}
