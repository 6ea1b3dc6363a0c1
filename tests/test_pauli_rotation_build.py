"""What the compiler made of the general gates' kernels -- K12 (one-qubit gate), K13 (two-qubit gate), K14 (Pauli expectation
value) and K15 (Pauli rotation; its own two tests came first and give the file its name): every instantiation there, without
scratch, with 16-B amplitude accesses, without FMA, and with the accumulator's "0.0 +" (q_row, and K14's leaf) still in it.
Host only: hipcc cross-compiles."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# <SHAPE, FULL>: no partner / inside the tile / another tile; the partial tile of n < 12 never has a partner in another tile
WANT = {(0, 0), (0, 1), (1, 0), (1, 1), (2, 1)}


@pytest.fixture(scope="module")
def isa():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "quantumcomputer_amd", "csrc"), "-s", "isa"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return open(os.path.join(ROOT, "quantumcomputer_amd", "libqcx.gfx950.s")).read()


def inst(name):
    m = re.match(r"_ZN3qcx11k_pauli_rotILi(\d)ELb([01])EE", name)
    return (int(m.group(1)), int(m.group(2))) if m else None


def test_every_instantiation_without_scratch(isa):
    meta = {inst(m.group(1)): (int(m.group(2)), int(m.group(3)))
            for m in re.finditer(r"\.name:\s*(\S*k_pauli_rot\S*)\s.*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+)", isa, re.S)}
    assert set(meta) == WANT, sorted(meta)
    for key, (scratch, vgpr) in meta.items():
        assert scratch == 0, (key, scratch)
        assert vgpr <= 256, (key, vgpr)                              # at least two workgroups' waves per SIMD: what 64 KiB of LDS allow


def test_accesses_and_arithmetic(isa):
    funcs = {m.group(1): isa[m.start():isa.find(".Lfunc_end", m.start())] for m in re.finditer(r"^(_Z\w+):", isa, re.M)}
    bodies = {inst(name): body for name, body in funcs.items() if inst(name)}
    assert set(bodies) == WANT, sorted(bodies)
    for key, body in bodies.items():
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, key
        assert not re.search(r"global_(load|store)_dword(x2)? ", body), key          # nothing narrower than an amplitude
        assert not re.search(r"v_fma_f64|v_fmac_f64|v_pk_fma_f64", body), key
        assert re.search(r"v_add_f64 v\[\d+:\d+\], v\[\d+:\d+\], 0\b", body), key      # the accumulator's start survives
        assert ("ds_read_b128" in body) == (key[0] == 1), key                        # LDS only where the partner is inside the tile


# ---- all four families ------------------------------------------------------------------------------------------------------
# kernel -> its template-argument tuples (bools as 0 / 1), as the launchers of qcx_api.hip instantiate them
PAULI_FORMS = {(0, 0), (0, 1), (1, 0), (1, 1), (2, 1)}
FAMILIES = {
    "k_u_pair": {(1, 0, 0, 64), (1, 1, 0, 64), (1, 0, 1, 64), (1, 1, 1, 64), (2, 0, 0, 64), (2, 1, 0, 64)},      # <PPT, NT, CTL, BLOCK>
    "k_u_wave": {(q, r, 1, 256) for r in (2, 4, 8) for q in range(9) if q < {2: 7, 4: 8, 8: 9}[r]},              # <Q, R, NT, BLOCK>
    "k_cu_lines": {(0,), (1,)},                                                                                 # <LOWQ>
    "k_u2_quad": {(nt, ctl, 64) for nt in (0, 1) for ctl in (0, 1)},                                            # <NT, CTL, BLOCK>
    "k_u2_lines": {(ns, nt) for ns in (0, 1, 2) for nt in (0, 1)},                                              # <NS, NT>
    "k_pauli_leaves": PAULI_FORMS,                                                                              # <SHAPE, FULL>
    "k_pauli_rot": PAULI_FORMS,
}
# An amplitude is one 16-B access.  The two narrower accesses there are, both of a double that is no amplitude:
#   k_pauli_leaves stores a tile's sum, dst[t] (two of them where a unit is a pair of tiles)
#   k_u2_lines<2, NT> picks the lane's own matrix row with selects; the compiler reads the row's eight components from the
#   kernel-argument segment with vector loads
NARROW_OK = {"k_pauli_leaves": ("store", lambda key: 2 if key[0] == 2 else 1), "k_u2_lines": ("load", lambda key: 8 if key[0] == 2 else 0)}


@pytest.fixture(scope="module")
def family_bodies(isa):
    """(kernel, template arguments) -> (function text, private_segment_fixed_size)"""
    scratch = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s*(_Z\S+)\s.*?\.private_segment_fixed_size:\s*(\d+)", isa, re.S)}
    out = {}
    for m in re.finditer(r"^(_ZN3qcx\d+(k_\w+?)I((?:L[ib]\d+E)+)E\w*):", isa, re.M):
        if m.group(2) in FAMILIES:
            key = (m.group(2), tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(3))))
            out[key] = (isa[m.start():isa.find(".Lfunc_end", m.start())], scratch[m.group(1)])
    return out


@pytest.mark.parametrize("kernel", sorted(FAMILIES))
def test_general_gate_kernels(family_bodies, kernel):
    got = {key[1]: v for key, v in family_bodies.items() if key[0] == kernel}
    assert set(got) == FAMILIES[kernel], sorted(got)
    for key, (body, scratch) in got.items():
        assert scratch == 0, (kernel, key, scratch)
        assert not re.search(r"v_fma_f64|v_fmac_f64|v_pk_fma_f64", body), (kernel, key)
        assert re.search(r"v_add_f64 v\[\d+:\d+\], v\[\d+:\d+\], 0\b", body), (kernel, key)          # the accumulator's start survives
        assert "global_load_dwordx4" in body, (kernel, key)
        assert ("global_store_dwordx4" in body) == (kernel != "k_pauli_leaves"), (kernel, key)    # (K14 writes no amplitude)
        narrow = re.findall(r"global_(load|store)_(?:dword|dwordx2|dwordx3|u?short|[us]?byte)(?:_d16\w*)? ", body)
        what, count = NARROW_OK.get(kernel, ("", lambda key: 0))
        assert narrow == [what] * count(key), (kernel, key, narrow)
        if narrow:
            assert len(re.findall(r"global_%s_dwordx2 " % what, body)) == len(narrow), (kernel, key)      # each of them a double
