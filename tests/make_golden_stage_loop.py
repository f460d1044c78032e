"""Records tests/golden/stage_loop_parent.npz, the fixture of tests/test_solver_stage_loop_cpu.py (CPU only, no GPU).

The fixture holds what the host emulation of the solver kernel (tests/emu) computed for a handful of short-horizon members BEFORE the
backward sweep became one resident stage loop (elimination inlined, lane constants formed once per sweep, context in scalar registers):
x, lam_g, iters, status, kkt and the sweep counters.  The new loop must reproduce them bit for bit, so the file is recorded ONCE, from an
emulation library built from the commit that precedes the change:

    git worktree add /tmp/parent <that commit> && make -C /tmp/parent/landing-controller_amd/csrc emu
    python tests/make_golden_stage_loop.py /tmp/parent/tests/emu/liblanding_emu.so

The cases (CASES below; the test runs the same list) are the horizons at which the loop is shortest:
  n2    N = 2: the last stage (12 controls, out of line) and ONE stage of the loop
  n4    N = 4: first, middle, penultimate and last stage type, three trips of the loop
  n5rc  N = 5, running-cost form (its gradient is added to gamma when the tile is fetched; rc_on travels in a scalar register); no sweep
        of these members is abandoned within the limit
Where a sweep is abandoned follows from the counters of a member: with F = attempted - ok abandoned sweeps among its S sweeps, the
S - F complete ones account for (N + 1) eliminations each (N stages + the foot block of stage 0) and the rest, `partial`, is what the
abandoned ones attempted: 1 each for a sweep given up at the last stage, 2..N at a stage of the loop, N + 1 at the foot block.  So
partial < 2 F shows a sweep abandoned at the last stage, (partial - F) % N != 0 one abandoned inside the loop (ones and N + 1s alone cannot
add up to it), partial > N F one abandoned at the foot block.  `--scan A:B` prints these for the seeds A..B-1 of every case instead of writing the file.
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stage_loop_parent.npz")
KEYS = ("x", "lam_g", "iters", "status", "kkt")
RC = dict(QX=[0, 0, 10, 10, 10, 0, 1, 1, 1, 1, 1, 1], Qc=[1, 1, 1], Qf=[1e-4, 1e-4, 1e-4], f_ref=[0, 0, 20.0])
# name: (N, seed of problem.make_batch, members, running cost); every case stops at LIMIT iterations, feasibility phase off (short horizons
# do not converge: the limit keeps the emulation to seconds; n2 and n4 reach iterations whose first sweeps are abandoned within it, n5rc does
# not -- all its sweeps are complete, it covers the running-cost path of the loop)
CASES = {
    "n2": (2, 1, 4, None),
    "n4": (4, 1, 4, None),
    "n5rc": (5, 1, 4, RC),
}
LIMIT = 16
PH_NFACT, PH_NSTAGE_OK, PH_NSTAGE = 8, 11, 13      # profile buffer: sweeps; stage eliminations that succeeded / were attempted


def run_case(lib_path, name, seed=None, profile=True):
    """outputs of one case + per member [sweeps, eliminations attempted, succeeded] (zeros without the profile buffer)"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    capi, problem = importlib.import_module("landing-controller_amd.capi"), importlib.import_module("landing-controller_amd.problem")
    N, seed0, B, rc = CASES[name]
    L = capi.LandingLib(N, lib_path=lib_path, run_cost=rc) if rc else capi.LandingLib(N, lib_path=lib_path)
    P, X0, _, _ = problem.make_batch(B, N, 0.6, seed=seed0 if seed is None else seed)
    o = L.default_opts()
    o.max_iter = LIMIT
    o.feas_phase = 0
    prof = np.zeros((B, 16))
    if profile:
        L.lib.landing_set_profile_buffer(L.ctx, prof.ctypes.data)
    r = L.solve_host(P, X0, o)
    L.lib.landing_set_profile_buffer(L.ctx, None)
    out = {k: np.asarray(r[k]).copy() for k in KEYS}
    L.close()
    return out, np.stack([prof[:, PH_NFACT], prof[:, PH_NSTAGE], prof[:, PH_NSTAGE_OK]], axis=1).astype(np.int64)


def abandoned(cov, N):
    """per member: (abandoned sweeps F, eliminations the abandoned sweeps attempted)"""
    F = cov[:, 1] - cov[:, 2]
    return F, cov[:, 1] - (cov[:, 0] - F) * (N + 1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", help="emulation library built from the commit before the stage loop")
    ap.add_argument("--scan", default="", help="A:B -- print the counters of the seeds A..B-1 only, write nothing")
    a = ap.parse_args()
    if a.scan:
        lo, hi = (int(v) for v in a.scan.split(":"))
        for name in CASES:
            for seed in range(lo, hi):
                out, cov = run_case(os.path.abspath(a.lib), name, seed)
                F, part = abandoned(cov, CASES[name][0])
                print("%-5s seed %3d status %s iters %s sweeps %s abandoned %s partial %s" % (name, seed, out["status"].tolist(), out["iters"].tolist(), cov[:, 0].tolist(), F.tolist(), part.tolist()))
        sys.exit(0)
    data = {}
    for name in CASES:
        out, cov = run_case(os.path.abspath(a.lib), name)
        F, part = abandoned(cov, CASES[name][0])
        print("%-5s status %s iters %s sweeps %s abandoned %s partial %s" % (name, out["status"].tolist(), out["iters"].tolist(), cov[:, 0].tolist(), F.tolist(), part.tolist()))
        for k in KEYS:
            data[name + "_" + k] = out[k]
        data[name + "_cov"] = cov
    np.savez_compressed(GOLDEN, **data)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
