"""Records tests/golden/between_sweeps_parent.npz, the fixture of tests/test_solver_between_sweeps_cpu.py (CPU only, no GPU).

The fixture holds what the host emulation of the solver kernel (tests/emu) computed for a handful of members BEFORE the phases between
the two sweeps were changed (the derivative phase reads the multipliers from a copy in LDS, laid over [G | P | A1 | A^], at horizons up
to 44): x, f, lam_g, iters, status, kkt, the sweep counters and the accept counters of the emulation build.  None of that
changes an operand or the order of a sum, so the file is recorded ONCE, from an emulation library built from the commit that precedes
the change:

    git worktree add /tmp/parent <that commit> && make -C /tmp/parent/landing-controller_amd/csrc emu
    python tests/make_golden_between_sweeps.py /tmp/parent/tests/emu/liblanding_emu.so

The cases (CASES below; the test runs the same list):
  n2, n3, n6   short horizons, four members: the copy's last stage (80 rows) sits one, two or five strides behind the boundary rows
  n5rc         N = 5, running-cost form
  n44, n45     both sides of the limit of the LDS copy (36 + 105 N <= 4 736 doubles): N = 44 fills it to 80 doubles, N = 45 reads the
               workspace as before; two members each
Every case runs with the feasibility phase ON and an iteration limit, so a member that has not converged at the limit goes on inside the
phase (at most three times the limit in all).  COVER lists what the accept counters of the cases must show between them: a swap accept of
a fused first trial, a back-tracked line search, a slack-correction accept and steps inside the feasibility phase.
"""
import argparse
import ctypes as C
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "between_sweeps_parent.npz")
KEYS = ("x", "f", "lam_g", "iters", "status", "kkt")
RC = dict(QX=[0, 0, 10, 10, 10, 0, 1, 1, 1, 1, 1, 1], Qc=[1, 1, 1], Qf=[1e-4, 1e-4, 1e-4], f_ref=[0, 0, 20.0])
# name: (N, seed of problem.make_batch, members, running cost, iteration limit)
CASES = {
    "n2": (2, 9, 4, None, 12),
    "n3": (3, 9, 4, None, 12),
    "n5rc": (5, 9, 4, RC, 12),
    "n6": (6, 9, 4, None, 12),
    "n44": (44, 1, 2, None, 4),
    "n45": (45, 1, 2, None, 4),
}
PH_NFACT, PH_NSTAGE_OK, PH_NSTAGE = 8, 11, 13      # profile buffer: sweeps; stage eliminations that succeeded / were attempted
FAST, FAST_CLIP, FIRST_REJECTED, BACKTRACK, CORR, FALLBACK, FEAS = range(7)      # landing_emu_accept_counts
COVER = {"fused accept": (FAST, FAST_CLIP), "back-tracked line search": (BACKTRACK,), "slack-correction accept": (CORR,), "feasibility phase": (FEAS,)}


def run_case(lib_path, name, case=None):
    """outputs of one case, per member [sweeps, eliminations attempted, succeeded] and the accept counters of the emulation build"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    capi, problem = importlib.import_module("landing-controller_amd.capi"), importlib.import_module("landing-controller_amd.problem")
    N, seed, B, rc, limit = case or CASES[name]
    L = capi.LandingLib(N, lib_path=lib_path, run_cost=rc) if rc else capi.LandingLib(N, lib_path=lib_path)
    P, X0, _, _ = problem.make_batch(B, N, 0.6, seed=seed)
    o = L.default_opts()
    o.max_iter = limit
    o.feas_phase = 1
    prof = np.zeros((B, 16))
    L.lib.landing_set_profile_buffer(L.ctx, prof.ctypes.data)
    r = L.solve_host(P, X0, o)
    L.lib.landing_set_profile_buffer(L.ctx, None)
    acc = np.zeros((B, 7), dtype=np.int32)
    for m in range(B):
        assert L.lib.landing_emu_accept_counts(C.c_int(m), acc[m].ctypes.data_as(C.POINTER(C.c_int))) == 0
    out = {k: np.asarray(r[k]).copy() for k in KEYS}
    L.close()
    return out, np.stack([prof[:, PH_NFACT], prof[:, PH_NSTAGE], prof[:, PH_NSTAGE_OK]], axis=1).astype(np.int64), acc.astype(np.int64)


# ---- the device fixture of tests/test_gpu_solver_between_sweeps.py: full solves (default options) of 8 members per horizon by the PRODUCT library of the
# commit before the change, on the MI355X:   python tests/make_golden_between_sweeps.py --gpu <parent's liblanding_mi355x.so>
# Two files, because x and lam_g of 8 members at N = 44 and 45 alone are 0.8 MB: the long pair of horizons has a file of its own.
GPU_GOLDEN = {"short": os.path.join(ROOT, "tests", "golden", "between_sweeps_gpu.npz"), "long": os.path.join(ROOT, "tests", "golden", "between_sweeps_gpu_long.npz")}
GPU_HORIZONS = {"short": (2, 3, 5, 6, 40), "long": (44, 45)}
GPU_B = 8


def gpu_batch(N):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("landing-controller_amd.problem").make_batch(GPU_B, N, 0.6, seed=700 + N)[:2]


def gpu_solve(N, lib_path=None):
    """x, f, lam_g, iters, status, kkt of the horizon's batch: default options, to the end"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    L = importlib.import_module("landing-controller_amd.capi").LandingLib(N, device=0, lib_path=lib_path)
    P, X0 = gpu_batch(N)
    r = L.solve_host(P, X0, L.default_opts())
    out = {k: np.asarray(r[k]).copy() for k in KEYS}
    L.close()
    return out


def record_gpu(lib_path, out_dir):
    for part, horizons in GPU_HORIZONS.items():
        data = {}
        for N in horizons:
            out = gpu_solve(N, lib_path)
            print("N %-2d status %s iters %s" % (N, out["status"].tolist(), out["iters"].tolist()))
            data.update({"n%d_%s" % (N, k): out[k] for k in KEYS})
        path = os.path.join(out_dir, os.path.basename(GPU_GOLDEN[part])) if out_dir else GPU_GOLDEN[part]
        np.savez_compressed(path, **data)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", help="library built from the commit before the change: the emulation, or with --gpu the product library")
    ap.add_argument("--gpu", action="store_true", help="record the device fixture (needs the MI355X)")
    ap.add_argument("--out-dir", default=None, help="with --gpu: write the two files there instead of tests/golden")
    a = ap.parse_args()
    if a.gpu:
        record_gpu(os.path.abspath(a.lib), a.out_dir)
        sys.exit(0)
    data, total = {}, np.zeros(7, dtype=np.int64)
    for name in CASES:
        out, cov, acc = run_case(os.path.abspath(a.lib), name)
        print("%-5s status %s iters %s sweeps %s accepts %s" % (name, out["status"].tolist(), out["iters"].tolist(), cov[:, 0].tolist(), acc.tolist()))
        for k in KEYS:
            data[name + "_" + k] = out[k]
        data[name + "_cov"], data[name + "_acc"] = cov, acc
        total += acc.sum(axis=0)
    for what, slots in COVER.items():
        assert total[list(slots)].sum() > 0, "no case shows a " + what
    np.savez_compressed(GOLDEN, **data)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
