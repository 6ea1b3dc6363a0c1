"""What the compiler makes of k_pauli_leaves_batch (K14b): every form the launcher instantiates -- <SHAPE, FULL, ODD> --, without
scratch, without FMA, with the root's "0.0 +" still in it, the amplitudes as 16-B loads, and no term's tree in LDS.
Host only: hipcc cross-compiles the kernel header with the library's flags and these instantiations alone."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quantumcomputer_amd", "csrc")
# <SHAPE, FULL> as k_pauli_leaves has them, each with and without t_odd
WANT = {(s, f, o) for s, f in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 1)) for o in (0, 1)}
ARGS = "const amp_t *, double *, uint64_t, uint64_t, unsigned, uint64_t, unsigned, PauliBatchTerms"


def make_var(name):
    txt = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^%s\s*\?=\s*(.*)$" % name, txt, re.M).group(1).strip()


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    d = tmp_path_factory.mktemp("k14b")
    src = ['#include <hip/hip_runtime.h>', '#include "qcx_kernels.h"', "namespace qcx {"]
    for s, f, o in sorted(WANT):
        src.append("template __global__ void k_pauli_leaves_batch<%d, %s, %s>(%s);" % (s, "true" if f else "false", "true" if o else "false", ARGS))
    src.append("}")
    (d / "inst.hip").write_text("\n".join(src) + "\n")
    flags = make_var("FLAGS").replace("$(ARCH)", make_var("ARCH")).split()
    r = subprocess.run([make_var("HIPCC"), *flags, "-I", CSRC, "--cuda-device-only", "-S", "-o", str(d / "inst.s"), str(d / "inst.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return (d / "inst.s").read_text()


def form(name):
    m = re.match(r"_ZN3qcx20k_pauli_leaves_batchILi(\d)ELb([01])ELb([01])EE", name)
    return tuple(int(v) for v in m.groups()) if m else None


def test_every_form_without_scratch(isa):
    meta = {}
    for entry in re.split(r"\n  - \.", isa[isa.index("amdhsa.kernels:"):]):                # one entry per kernel, its fields in any order
        name = re.search(r"\.name:\s*(\S*k_pauli_leaves_batch\S*)", entry)
        if name:
            meta[form(name.group(1))] = tuple(int(re.search(r"\.%s:\s*(\d+)" % f, entry).group(1))
                                              for f in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count"))
    assert set(meta) == WANT, sorted(meta)
    for key, (lds, scratch, vgpr) in meta.items():
        assert scratch == 0, (key, scratch)
        # one padded tile -- of amplitudes in the exchange shape (17 to a row of 16), else of t values, t_odd's beside t_even's (18
        # doubles to a row) -- and 32 terms' four wave sums: what ONE transposition a tile needs, whatever the number of terms
        tile = 256 * 17 * 16 if key[0] == 1 else 256 * 18 * 8 * (2 if key[2] else 1)
        assert lds == tile + 32 * 4 * 8, (key, lds)
        assert vgpr <= 512, (key, vgpr)


def test_arithmetic_and_accesses(isa):
    funcs = {m.group(1): isa[m.start():isa.find(".Lfunc_end", m.start())] for m in re.finditer(r"^(_Z\w+):", isa, re.M)}
    bodies = {form(name): body for name, body in funcs.items() if form(name)}
    assert set(bodies) == WANT, sorted(bodies)
    for key, body in bodies.items():
        assert not re.search(r"v_fma_f64|v_fmac_f64|v_pk_fma_f64", body), key
        assert re.search(r"v_add_f64 v\[\d+:\d+\], v\[\d+:\d+\], 0\b", body), key      # the root's 0.0 + survives
        assert "global_load_dwordx4" in body and "global_store_dwordx4" not in body, key
        assert not re.search(r"global_load_dword(x2)? ", body), key                    # nothing narrower than an amplitude is read
        assert len(re.findall(r"global_store_dwordx2 ", body)) == (2 if key[0] == 2 else 1), key     # a term's root, to both tiles of a pair
        assert "_dpp" in body and "ds_bpermute_b32" in body, key                       # the lane levels cross lanes, not LDS
        assert len(re.findall(r"s_barrier", body)) == 2, key                           # a tile's two barriers, none of them per term
