"""Records tests/golden/stage_layout_parent.npz, the fixture of tests/test_solver_stage_layout_cpu.py (CPU only, no GPU).

The fixture holds what the host emulation of the solver kernel (tests/emu) computed for a handful of members BEFORE the operand
arrays of the backward sweep were laid out in elimination order (G with gamma as its spare column, p in P, b in A^): x, lam_g, iters,
status and kkt.  The re-laid kernel must reproduce them bit for bit, so the file is recorded ONCE, from an emulation library built
from the commit that precedes the change:

    git worktree add /tmp/parent <that commit> && make -C /tmp/parent/landing-controller_amd/csrc emu
    python tests/make_golden_stage_layout.py /tmp/parent/tests/emu/liblanding_emu.so

The cases (CASES below; the test runs the same list):
  short   N = 3: first, penultimate and last stage only -- no stage of the resident middle type repeats
  mid     N = 6, iteration limit 7, no feasibility phase: a short horizon whose inner stages are all of the middle type
  n20     N = 20, the defaults
  rc      N = 20, running-cost form (its gradient is added to gamma when the tile is fetched)
  feas    N = 20, iteration limit 12: the members enter the feasibility phase, then the solve restarts
`--scan` prints, per member, the counters the test asserts its coverage with: sweeps attempted / succeeded (a failed one is
a delta_w retry) and the steps taken inside the feasibility phase.
"""
import argparse
import ctypes as C
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stage_layout_parent.npz")
KEYS = ("x", "lam_g", "iters", "status", "kkt")
RC = dict(QX=[0, 0, 10, 10, 10, 0, 1, 1, 1, 1, 1, 1], Qc=[1, 1, 1], Qf=[1e-4, 1e-4, 1e-4], f_ref=[0, 0, 20.0])
# name: (N, seed of problem.make_batch, members, running cost, iteration limit (0 = default), feasibility phase)
CASES = {
    "short": (3, 4, 2, None, 0, 1),
    "mid": (6, 3, 2, None, 7, 0),
    "n20": (20, 1, 2, None, 0, 1),
    "rc": (20, 2, 2, RC, 0, 1),
    "feas": (20, 5, 2, None, 12, 1),
}
FEAS_SLOT = 6                               # landing_emu_accept_counts: steps accepted inside the feasibility phase
PH_NSTAGE_OK, PH_NSTAGE = 11, 13            # profile buffer: stage eliminations that succeeded / were attempted


def run_case(lib_path, name):
    """outputs of one case + per member (sweeps' stage eliminations attempted, succeeded, feasibility-phase steps)"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    capi, problem = importlib.import_module("landing-controller_amd.capi"), importlib.import_module("landing-controller_amd.problem")
    N, seed, B, rc, lim, feas = CASES[name]
    L = capi.LandingLib(N, lib_path=lib_path, run_cost=rc) if rc else capi.LandingLib(N, lib_path=lib_path)
    P, X0, _, _ = problem.make_batch(B, N, 0.6, seed=seed)
    o = L.default_opts()
    if lim:
        o.max_iter = lim
    o.feas_phase = feas
    prof = np.zeros((B, 16))
    L.lib.landing_set_profile_buffer(L.ctx, prof.ctypes.data)
    r = L.solve_host(P, X0, o)
    L.lib.landing_set_profile_buffer(L.ctx, None)
    acc = np.zeros((B, 7), dtype=np.int32)
    for m in range(B):
        assert L.lib.landing_emu_accept_counts(C.c_int(m), acc[m].ctypes.data_as(C.POINTER(C.c_int))) == 0
    out = {k: np.asarray(r[k]).copy() for k in KEYS}
    L.close()
    return out, np.stack([prof[:, PH_NSTAGE], prof[:, PH_NSTAGE_OK], acc[:, FEAS_SLOT]], axis=1).astype(np.int64)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", help="emulation library built from the commit before the layout change")
    ap.add_argument("--scan", action="store_true", help="print the coverage counters only, write nothing")
    a = ap.parse_args()
    data = {}
    for name in CASES:
        out, cov = run_case(os.path.abspath(a.lib), name)
        print("%-6s status %s iters %s  [attempted, succeeded, feasibility steps] %s" % (name, out["status"].tolist(), out["iters"].tolist(), cov.tolist()))
        for k in KEYS:
            data[name + "_" + k] = out[k]
    if not a.scan:
        np.savez_compressed(GOLDEN, **data)
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
