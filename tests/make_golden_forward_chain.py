"""Records tests/golden/forward_chain_parent.npz, the fixture of tests/test_solver_forward_chain_cpu.py (CPU only, no GPU).

The fixture holds what the host emulation of the solver kernel (tests/emu) computed for a handful of short-horizon members BEFORE the
forward recursion and the assembly hooks of the backward sweep were taken off the LDS pipe (lane constants and
the record base of the forward loop hoisted, the bias of a row read with the row, the two cases of a row as selects; the assembly's term
and combine words fetched one block step early; the 8-lane sum behind lane_sum8_head): x, lam_g, iters, status, kkt and the sweep counters.
None of that changes an operand or the order of a sum, so the file is recorded ONCE, from an emulation library built from the commit that
precedes the change:

    git worktree add /tmp/parent <that commit> && make -C /tmp/parent/landing-controller_amd/csrc emu
    python tests/make_golden_forward_chain.py /tmp/parent/tests/emu/liblanding_emu.so

The cases (CASES below; the test runs the same list) are horizons that are no multiple of the forward loop's unroll factor 4, so the loop
runs its clamped prefetches (stages past N - 1 re-read the last record) and its `k < N` guards:
  n2    N = 2: half a trip of the unrolled loop; stage 1 is the last one (its c+ rows are 0)
  n3    N = 3: one trip less one stage
  n5rc  N = 5, running-cost form: one full trip and the first stage of a second one; the gradient of the running cost travels through the
        assembly hooks (stored one block step earlier than before)
  n6    N = 6: one full trip and a half
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "forward_chain_parent.npz")
KEYS = ("x", "lam_g", "iters", "status", "kkt")
RC = dict(QX=[0, 0, 10, 10, 10, 0, 1, 1, 1, 1, 1, 1], Qc=[1, 1, 1], Qf=[1e-4, 1e-4, 1e-4], f_ref=[0, 0, 20.0])
# name: (N, seed of problem.make_batch, members, running cost); every case stops at LIMIT iterations, feasibility phase off
CASES = {
    "n2": (2, 1, 4, None),
    "n3": (3, 1, 4, None),
    "n5rc": (5, 1, 4, RC),
    "n6": (6, 1, 4, None),
}
LIMIT = 12
PH_NFACT, PH_NSTAGE_OK, PH_NSTAGE = 8, 11, 13      # profile buffer: sweeps; stage eliminations that succeeded / were attempted


def run_case(lib_path, name, profile=True):
    """outputs of one case + per member [sweeps, eliminations attempted, succeeded] (zeros without the profile buffer)"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    capi, problem = importlib.import_module("landing-controller_amd.capi"), importlib.import_module("landing-controller_amd.problem")
    N, seed, B, rc = CASES[name]
    L = capi.LandingLib(N, lib_path=lib_path, run_cost=rc) if rc else capi.LandingLib(N, lib_path=lib_path)
    P, X0, _, _ = problem.make_batch(B, N, 0.6, seed=seed)
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", help="emulation library built from the commit before the change")
    a = ap.parse_args()
    data = {}
    for name in CASES:
        out, cov = run_case(os.path.abspath(a.lib), name)
        print("%-5s status %s iters %s sweeps %s attempted %s ok %s" % (name, out["status"].tolist(), out["iters"].tolist(), cov[:, 0].tolist(), cov[:, 1].tolist(), cov[:, 2].tolist()))
        for k in KEYS:
            data[name + "_" + k] = out[k]
        data[name + "_cov"] = cov
    np.savez_compressed(GOLDEN, **data)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
