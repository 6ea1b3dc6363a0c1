"""What the compiler made of K15 (k_pauli_rot, the kernel of qcx_pauli_rotation): every instantiation without scratch, with
16-B amplitude accesses, without FMA, and with the accumulator's "0.0 +" still in it.  Host only: hipcc cross-compiles."""
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
