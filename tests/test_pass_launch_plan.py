"""CPU: the launch of a fused pass as a plan (pass_launch_plan in csrc/qcx_fuse.inc.h; qcx_pass_launch_plan in include/qcx_plan.h):
which kernel instantiation, grid, block, dynamic LDS layout, and the FusePass fields the launch fills in -- or the refusal.

The expectation is the commit BEFORE the launch became "plan, then dispatch": there launch_pass chose among the ~70
instantiations with macros, ifs and switches between its hipLaunchKernelGGL calls.  A copy of that commit with those calls
replaced by a recorder (kernel as its demangled symbol, grid, block, LDS bytes, the FusePass handed over) answered the
enumeration of tests/pass_launch_cases.py under each knob set; tests/golden/pass_launch_digests.json holds one SHA-256 per knob
set over the canonical lines, a readable sample of lines, and the kernels reached.  The expanding-store predicate (xp_ok) of
a line is that commit's pass_is_x8.  (cam_ctl_local[3] entered that launch as the planner's emit set it: the multiply scratch's
size; it is now computed with the rest of the layout.)"""
import ctypes as C
import hashlib
import json
import os
import re

import pytest

import pass_launch_cases as plc

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "pass_launch_digests.json")))

# every instantiation of the pass kernels (QCX_PASS_KERNELS in csrc/qcx_fuse.inc.h), restated
ROUNDS = [(8, "false", 2, "true"), (6, "false", 2, "true"), (6, "false", 1, "true"), (7, "false", 0, "true"), (6, "false", 0, "true")] + \
         [(o, c, s, "false") for o, s in ((8, 2), (6, 2), (6, 1), (7, 0), (6, 0)) for c in ("true", "false")]
INSTANTIATIONS = sorted(
    [f"k_fused<{b}, {t}, {d}>" for b, t in ((1024, 12), (512, 11), (256, 10), (256, 9)) for d in ("true", "false")] +
    [f"k_fused<64, {t}, false>" for t in (8, 7, 6, 5)] + ["k_fused<256, 0, false>"] +
    [f"k_fused_rounds<{b}, {t}, {o}, {c}, {s}, {g}>" for b, t in ((1024, 12), (512, 11), (256, 10)) for o, c, s, g in ROUNDS] +
    [f"k_fused_q3<512, 12, 4, {e}, {g}>" for e in ("true", "false") for g in ("true", "false")] +
    [f"k_fused_x8<{b}, {t}, {g}, false>" for b, t in ((512, 12), (256, 11), (128, 10)) for g in ("true", "false")] +
    ["k_fused_x8<512, 12, false, true>"] + [f"k_gen_cols<6, {t}>" for t in ("true", "false")])
# instantiations the enumeration does not reach, with the knob that would reach them
NOT_REACHED = {}

REFUSALS = ("fused pass: chained flag and buffers disagree", "expanding store on a pass that is not a k_fused_x8 pass",
            "fused pass: the addressing tables do not cover the", "radix-8 exact pass: unsupported shape", "radix-8 pass on a tile of",
            "chained pass without a rounds kernel")


@pytest.fixture()
def knob_guard(qc):
    old = {k: qc.lib().qcx_tune_get(k.encode()) for k in plc.KNOBS}
    yield old
    qc.tune(**old)


@pytest.fixture(scope="module")
def rows():
    return plc.cases()


def library_call(qc):
    from quantumcomputer_amd import _lib
    O = _lib.PassLaunchOut()
    pO, fn, last = C.addressof(O), qc.lib().qcx_pass_launch_plan, qc.lib().qcx_last_error

    def call(p):
        st = fn(p, pO)
        if st:
            return st, "", (), last().decode(), O.expanding_store_ok
        return 0, O.kernel.decode(), tuple(getattr(O, k) for k in plc.OUT_FIELDS), "", O.expanding_store_ok
    return call


def test_the_fixture_covers_the_launch():
    """depends on the fixture alone: five families, three LDS layouts, six refusals, the instantiations by name"""
    assert len(INSTANTIATIONS) == 71 and len(set(INSTANTIATIONS)) == 71
    reached = set(GOLDEN["kernels"])
    assert reached <= set(INSTANTIATIONS)
    assert {k[:k.index("<")] for k in reached} == {"k_fused", "k_fused_rounds", "k_fused_q3", "k_fused_x8", "k_gen_cols"}
    assert len(reached) >= 0.9 * len(INSTANTIATIONS)
    assert set(INSTANTIATIONS) - reached == set(NOT_REACHED)
    lines = [s["line"] for s in GOLDEN["sample"]]
    assert 24 <= len(lines) <= 60 and all(s["knobs"] in plc.KNOB_SETS for s in GOLDEN["sample"])
    tails = [ln.split(" | ")[2] for ln in lines]
    for r in REFUSALS:
        assert any(t.startswith("refused 4: " + r) for t in tails), r
    fams = {t[:t.index("<")] for t in tails if not t.startswith("refused")}
    # the three layouts: behind a tile the general areas (k_fused, k_fused_rounds, k_fused_q3), the radix-8 ones (k_fused_x8); behind columns
    assert fams == {"k_fused", "k_fused_rounds", "k_fused_q3", "k_fused_x8", "k_gen_cols"}
    assert any(" | xp_ok=1 | " in ln for ln in lines)
    assert set(GOLDEN["digests"]) == set(plc.KNOB_SETS) and GOLDEN["cases"] > 400000


def test_the_enumeration_is_the_recorded_one(rows):
    assert len(rows) == GOLDEN["cases"]
    # every rule of keep() leaves its slice: all axes' values survive
    for k, v in plc.VALUES:
        if k != "n_off":
            assert set(int(x) for x in set(rows[k].tolist())) == set(v), k
    assert set((rows["n"] - rows["T"]).tolist()) == {0, 2, 18}


@pytest.mark.parametrize("name", list(plc.KNOB_SETS))
def test_launch_plans_are_the_parents(qc, knob_guard, rows, name):
    """every line of the enumeration under one knob set: digest and sample lines"""
    qc.tune(**{k: plc.KNOB_SETS[name].get(k, v) for k, v in knob_guard.items()})
    lines = plc.answer_lines(rows, library_call(qc))
    have = set(lines)
    for s in GOLDEN["sample"]:
        if s["knobs"] == name:
            assert s["line"] in have, s["line"]
    assert hashlib.sha256("\n".join(lines).encode()).hexdigest() == GOLDEN["digests"][name]


def test_plan_actions_carry_the_launch(qc, knob_guard):
    """qcx_fusion_plan reports the launch of every pass; a stand-alone gate has none"""
    descs = [(0, q, 0, 0.0, 0.0, 0, 0) for q in range(14)] + [(2, 13, 0, 0.0, 0.0, 15, 7)]
    for mode in (1, 2, 5):
        actions, recs, nrec = qc.fusion_plan(14, 4, descs, mode)
        assert any(a.fused for a in actions)
        for a in actions:
            if not a.fused:
                assert (a.kernel, a.grid, a.block, a.lds_bytes) == (b"", 0, 0, 0)
                continue
            assert re.fullmatch(r"k_\w+<[\w, ]+>", a.kernel.decode()) and a.kernel.decode() in INSTANTIATIONS
            assert a.block in (64, 128, 256, 512, 1024) and 1 <= a.grid <= 1 << (14 - a.T) and (16 << a.T) <= a.lds_bytes <= 160 * 1024


def test_bad_arguments(qc):
    from quantumcomputer_amd import _lib
    O, I = _lib.PassLaunchOut(), _lib.PassLaunchIn(n=0, T=0)
    assert qc.lib().qcx_pass_launch_plan(C.byref(I), C.byref(O)) == 2
    assert qc.lib().qcx_pass_launch_plan(None, C.byref(O)) == 2
    I = _lib.PassLaunchIn(n=10, M=4, T=12, tables_cover=1)          # a tile larger than the register: its tables cannot cover
    assert qc.lib().qcx_pass_launch_plan(C.byref(I), C.byref(O)) == 4 and b"do not cover" in qc.lib().qcx_last_error()


def test_launch_plan_under_host_sanitizers(tmp_path):
    """tests/c/pass_launch_sanitize.cpp: the library's source around a main of its own, host side built under
    AddressSanitizer and UBSan (device code built normally), run over a slice of the enumeration with ordinary and hostile knobs (CPU only, its own process)"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "pass_launch_sanitize")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    host_only = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]      # the host side alone
    subprocess.run([hipcc, "-O1", "-g", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", *host_only, "-o", exe,
                    os.path.join(root, "tests", "c", "pass_launch_sanitize.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "pass_launch_sanitize ok" in r.stdout, r.stdout + r.stderr
