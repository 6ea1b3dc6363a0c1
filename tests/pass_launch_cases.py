"""The inputs of a fused pass's launch decision (qcx_pass_launch_plan, include/qcx_plan.h), enumerated, and the canonical line of
one answer.  tests/test_pass_launch_plan.py feeds the enumeration to the library and compares with the answers recorded from the
commit before the launch became "plan, then dispatch" (tests/golden/pass_launch_digests.json); the same enumeration produced those.

The enumeration is the cross product of VALUES below with n in {T, T + 2, T + 18}, pruned by the rules of keep() -- every rule
removes combinations that the launch REFUSES whatever the knobs, and keeps a slice of them (the `minor` inputs at their first
value), so that each refusal stays covered.  No combination that reaches a launch is pruned.
"""
import numpy as np

FIELDS = ("n", "M", "T", "rounds_form", "table_bytes", "has_cam", "xm_cnt", "dg_cnt", "dg_slim", "chained", "gen",
          "gen_tab_bytes", "zpad", "zskip", "xp_on", "tables_cover", "buffers_differ")         # qcx_pass_launch_in, in its order
DTYPE = np.dtype([(k, np.uint32) for k in FIELDS])

# the axes in canonical order (the first varies slowest); n_off: n = T + n_off
VALUES = [("T", range(5, 14)), ("dg_slim", range(4)), ("dg_cnt", (0, 3, 16)), ("gen", range(4)), ("has_cam", (0, 1)), ("rounds_form", (0, 1)),
          ("table_bytes", (0, 96)), ("xm_cnt", (0, 5)), ("chained", (0, 1)), ("zskip", (0, 2)), ("xp_on", (0, 1)), ("zpad", (6, 8)),
          ("gen_tab_bytes", (0, 64)), ("tables_cover", (1, 0)), ("buffers_differ", (0, 1)), ("n_off", (0, 2, 18)), ("M", (4, 12))]

KNOB_SETS = {
    "default": {},
    "ldsdma_0": {"fuse_ldsdma": 0},
    "rounds_occ_0": {"fuse_rounds_occ": 0},
    "rounds_occ_6": {"fuse_rounds_occ": 6},
    "tol_occ_8": {"fuse_tol_occ": 8},
    "x8t_0": {"fuse_x8t": 0},
    "streams_3_4": {"fuse_streams_log2": 3, "fuse_streams_pos": 4},
    "cols_waves_6": {"fuse_cols_waves": 6},
    "caps_1024": {"fuse_grid_cap": 1024, "fuse_x8_cap": 1024, "fuse_q3_cap": 1024, "fuse_q3_cap_exact": 1024, "fuse_cols_cap": 1024},
}
KNOBS = sorted({k for s in KNOB_SETS.values() for k in s})


def keep(c):
    """the pruning rules, on a dict of equally shaped arrays: True = the combination stays"""
    minor = (c["table_bytes"] == 0) & (c["xm_cnt"] == 0) & (c["zpad"] == 6) & (c["gen_tab_bytes"] == 0) & (c["M"] == 4) & (c["n_off"] == 2)
    refused = c["tables_cover"] == 0                                                    # tables that do not cover: refused
    refused |= (c["xp_on"] == 0) & (c["chained"] != c["buffers_differ"])                # chained flag against the buffers: refused
    # the expanding store outside a radix-8 pass on a 2^12 tile that is read, without multiplies or zskip: refused
    refused |= (c["xp_on"] == 1) & ((c["T"] != 12) | (c["gen"] != 0) | (c["has_cam"] != 0) | (c["zskip"] != 0) | (c["dg_slim"] < 2))
    # the exact walk on 8 amplitudes outside its shapes: refused
    refused |= (c["dg_slim"] == 3) & ((c["T"] < 10) | (c["T"] > 12) | (c["has_cam"] != 0) | (c["gen"] > 1) | (c["zskip"] != 0))
    # radix-8 fast rounds (not by columns) on another tile than 2^12: refused
    refused |= (c["dg_slim"] == 2) & (c["gen"] < 2) & (c["T"] != 12)
    return ~refused | minor


def cases():
    """the enumeration: a structured array (DTYPE) in canonical order"""
    out = []
    names = [k for k, _ in VALUES]
    for T in VALUES[0][1]:
        axes = [np.array([T], dtype=np.uint32)] + [np.array(list(v), dtype=np.uint32) for _, v in VALUES[1:]]
        grid = np.meshgrid(*axes, indexing="ij")
        c = {k: g.ravel() for k, g in zip(names, grid)}
        sel = keep(c)
        rows = np.zeros(int(sel.sum()), dtype=DTYPE)
        for k in FIELDS:
            rows[k] = (c["T"] + c["n_off"])[sel] if k == "n" else c[k][sel]
        out.append(rows)
    return np.concatenate(out)


def line(row, status, kernel="", fields=(), err="", xp_ok=0):
    """the canonical line of one answer.  fields: grid, block, lds_bytes, waves, xm_off, dg_lds_off, gen_lds_off, table_lds_off, dbg"""
    head = " ".join(str(int(v)) for v in row)
    if status:
        return f"{head} | xp_ok={int(xp_ok)} | refused {int(status)}: {err}"
    return f"{head} | xp_ok={int(xp_ok)} | {kernel} " + " ".join(str(int(v)) for v in fields)


OUT_FIELDS = ("grid", "block", "lds_bytes", "waves", "xm_off", "dg_lds_off", "gen_lds_off", "table_lds_off", "dbg")


def answer_lines(rows, call):
    """one line per row; call(pointer to the row's 17 uint32) -> (status, out struct with kernel / OUT_FIELDS / xp flag name, err text)"""
    base, step = rows.ctypes.data, rows.dtype.itemsize
    lines = []
    for i, row in enumerate(rows.tolist()):
        status, kernel, fields, err, xp_ok = call(base + i * step)
        lines.append(line(row, status, kernel, fields, err, xp_ok))
    return lines
