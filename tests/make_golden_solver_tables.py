"""Records tests/golden/solver_tables_parent.npz, the fixture of tests/test_solver_tables_cpu.py and tests/test_gpu_solver_tables.py.

The fixture pins the tables the solver kernel reads (landing_debug_solver_tables: ctab, ccomb, ctype, rterm and the ints c_ml, c_mid, rlen)
as the host code built them BEFORE build_tables was rewritten to produce them in one pass.  The rewrite must hand the kernel the same bytes,
so the file is recorded ONCE, from an emulation library built from the commit that precedes the rewrite (with the accessor added to it):

    git worktree add /tmp/parent <that commit> && make -C /tmp/parent/landing-controller_amd/csrc emu
    python tests/make_golden_solver_tables.py /tmp/parent/tests/emu/liblanding_emu.so

Per case it holds the SHA-256 and the byte length of each of the four tables, the three ints, and ctype in full -- not the tables themselves
(196 KB at N = 96).  The cases (CASES below; the tests run the same list):
  n2, n3    2 and 3 stage types, c_mid = 0: no stage of a type repeats
  n4, n6    the first horizon with a middle stage; the first where the middle type is the most frequent one (c_mid = 1)
  n20, n40, n96   ctab and ccomb no longer depend on N from N = 4 on: these exercise rterm and its 16-bit index fields
  rc3, rc20       the running-cost form, whose constants are further operands of the assembly
  ccc41     the running-cost form with the weights as parameters, at the horizon of the script it comes from
"""
import argparse
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "solver_tables_parent.npz")
TABLES = ("ctab", "ccomb", "ctype", "rterm")
SCALARS = ("c_ml", "c_mid", "rlen")
RC = dict(QX=[0, 0, 10, 10, 10, 0, 1, 1, 1, 1, 1, 1], Qc=[1, 1, 1], Qf=[1e-4, 1e-4, 1e-4], f_ref=[0, 0, 20.0])      # (make_golden_stage_layout.py's)
# name: (N, running cost, weights as parameters)
CASES = {
    "n2": (2, None, False), "n3": (3, None, False), "n4": (4, None, False), "n6": (6, None, False),
    "n20": (20, None, False), "n40": (40, None, False), "n96": (96, None, False),
    "rc3": (3, RC, False), "rc20": (20, RC, False), "ccc41": (41, RC, True),
}


def record(lib_path, name, device=0):
    """what the fixture holds of one case: {"<table>_sha256": hex digest, "<table>_bytes": length, "ctype": the array, "c_ml" ...: ints};
    lib_path None: the product library"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    capi = importlib.import_module("landing-controller_amd.capi")
    N, rc, ccc = CASES[name]
    L = capi.LandingLib(N, device=device, lib_path=lib_path, run_cost=rc, ccc_params=ccc)
    try:
        t = L.solver_tables()
    finally:
        L.close()
    out = {k: np.int64(t[k]) for k in SCALARS}
    for k in TABLES:
        out[k + "_sha256"] = np.str_(hashlib.sha256(t[k].tobytes()).hexdigest())
        out[k + "_bytes"] = np.int64(t[k].nbytes)
    out["ctype"] = t["ctype"]
    return out


def assert_equals_fixture(got, golden, name):
    """`got` (record()) holds every key the fixture has of case `name`, with equal values"""
    keys = [k[len(name) + 1:] for k in golden.files if k.startswith(name + "_")]
    assert sorted(keys) == sorted(got), keys
    for k in keys:
        assert np.array_equal(got[k], golden[name + "_" + k]), "%s: %s is %s, recorded %s" % (name, k, got[k], golden[name + "_" + k])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", help="emulation library built from the commit before the rewrite of build_tables")
    a = ap.parse_args()
    data = {}
    for name in CASES:
        rec = record(os.path.abspath(a.lib), name)
        print("%-6s" % name, {k: int(rec[k]) for k in SCALARS}, {k: int(rec[k + "_bytes"]) for k in TABLES}, "types", rec["ctype"].tolist()[:6], "...")
        for k, v in rec.items():
            data[name + "_" + k] = v
    np.savez_compressed(GOLDEN, **data)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
