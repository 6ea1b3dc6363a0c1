"""What the compiler made of k_gate_run (K12b / K13b, a run of one- and two-qubit gates in one pass): exactly the four
instantiations <LDS, FULL>, without scratch, within 256 VGPRs, with 64 KiB of LDS or none, with 16-B amplitude accesses and
nothing narrower, the gate records read with scalar loads, without FMA, with the accumulator's "0.0 +" (q_row) still in it, and
LDS and barriers only where a pass can hold a gate with a low target.  Host only: hipcc cross-compiles."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {(l, f) for l in (0, 1) for f in (0, 1)}                     # <LDS, FULL>


@pytest.fixture(scope="module")
def isa():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "quantumcomputer_amd", "csrc"), "-s", "isa"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return open(os.path.join(ROOT, "quantumcomputer_amd", "libqcx.gfx950.s")).read()


def inst(name):
    m = re.match(r"_ZN3qcx10k_gate_runILb([01])ELb([01])EE", name)
    return (int(m.group(1)), int(m.group(2))) if m else None


def test_every_instantiation_without_scratch(isa):
    meta = {}
    for entry in re.split(r"\n  - \.", isa[isa.index("amdhsa.kernels:"):]):                # one entry per kernel, its fields in any order
        name = re.search(r"\.name:\s*(\S*k_gate_run\S*)", entry)
        if name:
            meta[inst(name.group(1))] = tuple(int(re.search(r"\.%s:\s*(\d+)" % f, entry).group(1))
                                              for f in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count"))
    assert set(meta) == WANT, sorted(meta)
    for key, (lds, scratch, vgpr) in meta.items():
        assert scratch == 0, (key, scratch)
        assert vgpr <= 256, (key, vgpr)                              # two workgroups' waves per SIMD: what 64 KiB of LDS allow
        assert lds == (65536 if key[0] else 0), (key, lds)           # one tile of amplitudes, and nothing in a pass of hot targets


def test_accesses_and_arithmetic(isa):
    funcs = {m.group(1): isa[m.start():isa.find(".Lfunc_end", m.start())] for m in re.finditer(r"^(_Z\w+):", isa, re.M)}
    bodies = {inst(name): body for name, body in funcs.items() if inst(name)}
    assert set(bodies) == WANT, sorted(bodies)
    for key, body in bodies.items():
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, key
        # nothing narrower than an amplitude touches memory; the records are kernel arguments and come through the scalar cache
        assert not re.search(r"(global|flat)_(load|store)_(dword|dwordx2|dwordx3|u?short|[us]?byte)(_d16\w*)? ", body), key
        assert re.search(r"s_load_dwordx(2|4|8|16) ", body), key
        assert not re.search(r"v_fma_f64|v_fmac_f64|v_pk_fma_f64", body), key
        assert re.search(r"v_add_f64 v\[\d+:\d+\], v\[\d+:\d+\], 0\b", body), key      # the accumulator's start survives
        assert bool(re.search(r"\bds_(read|write|load|store)", body)) == (key[0] == 1), key      # LDS only where LDS is true
        assert ("s_barrier" in body) == (key[0] == 1), key
