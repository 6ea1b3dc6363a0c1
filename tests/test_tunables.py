"""The launch knobs (qcx_tune_set / qcx_tune_get): every knob of tests/golden/tunables.json is there with its recorded default,
and a value set is the value read back.  The table was read with qcx_tune_get from the build before the knob list became one
X-macro; a new knob adds a line to it.  The child process loads the library and never touches a device: defaults are what a
process starts with, and this one's knobs may have been turned by other tests."""
import json
import os
import subprocess
import sys

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tunables.json")

CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.qcx_tune_get.restype = ctypes.c_long
lib.qcx_tune_get.argtypes = [ctypes.c_char_p]
lib.qcx_tune_set.argtypes = [ctypes.c_char_p, ctypes.c_long]
names = json.load(open(sys.argv[2]))
defaults = {k: lib.qcx_tune_get(k.encode()) for k in names}
back = {}
for i, k in enumerate(names):
    assert lib.qcx_tune_set(k.encode(), 1000 + i) == 0, k
for i, k in enumerate(names):                       # (all set before any is read: no knob aliases another)
    back[k] = lib.qcx_tune_get(k.encode())
unknown = [lib.qcx_tune_set(b"no_such_knob", 1), lib.qcx_tune_get(b"no_such_knob")]
print(json.dumps({"defaults": defaults, "back": back, "unknown": unknown}))
"""


def test_every_knob_has_its_default_and_round_trips(qc):
    want = json.load(open(GOLD))
    r = subprocess.run([sys.executable, "-c", CHILD, qc.LIB_PATH, GOLD], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["defaults"] == want
    assert got["back"] == {k: 1000 + i for i, k in enumerate(want)}
    assert got["unknown"] == [2, -1]                 # QCX_BAD_ARGUMENTS, and -1 for a name that is no knob
