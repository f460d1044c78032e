"""CPU test (no GPU) of the fused first trial of the solver kernel's line search, through the host emulation (tests/emu).

In interior-point mode the first trial pass of an iteration also prepares s, zL, zU, y, Sigma, rho and the error sums of that trial point in the
shadow instance of the row arrays; if the line search takes the point as it stands, accepting it is a swap of instances.  A back-tracked line
search, the slack-correction accept, the fallback step and the feasibility phase keep the accept pass over the rows.  Three members (N = 20,
iteration limit 25, otherwise the defaults) cover all of it between them:
  * (seed 3, member 3): converges with every iteration accepted at its first trial point, with and without the clip rule in force;
  * (seed 1, member 0): one first trial rejected and then accepted with the slack correction; enters the feasibility phase at the limit;
  * (seed 1, member 3): back-tracked line searches, a slack-correction accept, clip rule, feasibility phase.
(0) the results are the SAME BITS as those of a run in which no trial pass is fused and every step goes through the accept pass over the rows
    (landing_emu_set_fused(0), emulation build only) -- the tolerances of (a) would not see, say, a dual step length without its cap in the fused
    pass; the emulation also aborts if the two instances ever disagree at a swap in an entry the fused pass does not write;
(a) the emulated kernel follows the CPU port -- same status, same iteration count, same point (tolerances of test_solver_cpu.py's
    test_emulated_kernel_follows_cpu_port); (b) landing_emu_accept_counts() -- counters that exist in the emulation build only -- shows which
    accept path every step took."""
import ctypes as C

import numpy as np
import pytest

from conftest import lc
from emu_support import build_emu

FAST, FAST_CLIP, FIRST_REJECTED, BACKTRACK, CORR, FALLBACK, FEAS = range(7)


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu()


def accept_counts(L, B):
    out = np.zeros((B, 7), dtype=np.int32)
    for m in range(B):
        assert L.lib.landing_emu_accept_counts(C.c_int(m), out[m].ctypes.data_as(C.POINTER(C.c_int))) == 0
    return out


def test_fused_first_trial_paths_follow_cpu_port(emu_lib, oracle_mod):
    N, K = 20, 25
    Pm = lc("problem")
    O = oracle_mod.Oracle(N)
    P1, X1, _, _ = Pm.make_batch(6, N, 0.6, seed=1)
    P3, X3, _, _ = Pm.make_batch(4, N, 0.6, seed=3)
    P, X0 = np.stack([P3[3], P1[0], P1[3]]), np.stack([X3[3], X1[0], X1[3]])
    L = lc("capi").LandingLib(N, lib_path=emu_lib)
    o = L.default_opts(); o.max_iter = K
    assert o.feas_phase == 1 and o.slack_corr > 0.0 and o.clip_k > 1 and o.dual_step_cap > 0.0
    prof = np.zeros((3, 16))      # the kernel's own counters (landing_set_profile_buffer; the timers read 0 in the emulation): slot 9 = trial points
    L.lib.landing_set_profile_buffer(L.ctx, prof.ctypes.data)
    g = L.solve_host(P, X0, o)
    L.lib.landing_set_profile_buffer(L.ctx, None)
    n = accept_counts(L, 3)
    trials = prof[:, 9].astype(int)
    # (0) equal bits without the fused pass
    L.lib.landing_emu_set_fused(C.c_int(0))
    try:
        g0 = L.solve_host(P, X0, o)
        n0 = accept_counts(L, 3)
    finally:
        L.lib.landing_emu_set_fused(C.c_int(1))
    assert not n0[:, [FAST, FAST_CLIP, FIRST_REJECTED]].any()      # the switch really took the fused pass out
    for k in ("x", "f", "lam_g", "status", "iters", "kkt"):
        assert np.array_equal(g[k], g0[k]), k
    c = oracle_mod.cpu_solve_batch(O, P, X0, threads=3, max_iter=K)
    print("status", g["status"], c["status"], "iters", g["iters"], c["iters"], "trial points", trials)
    print("accept counts (swap, swap under the clip rule, first trial rejected, back-tracked, slack correction, fallback, feasibility phase):\n", n)
    # (a) the kernel follows the port
    assert np.array_equal(g["status"], c["status"]) and np.array_equal(g["iters"], c["iters"])
    for b in range(3):
        dx, dl = np.max(np.abs(g["x"][b] - c["x"][b])), np.max(np.abs(g["lam_g"][b] - c["lam_g"][b]))
        print("member %d: |x - x_port| %.3e, |lam - lam_port| %.3e" % (b, dx, dl))
        assert dx < 1e-7 * max(1.0, np.max(np.abs(c["x"][b])))
        assert dl < 1e-6 * max(1.0, np.max(np.abs(c["lam_g"][b])))
    # (b) which path ran
    # the plain member: every line search took its first trial point and every one of them was accepted by a swap, with and without the clip rule
    # in force; no row-pass accept at all (its other iterations are restarts: no step is taken in them)
    assert g["status"][0] == 0
    assert n[0, FAST] > 0 and n[0, FAST_CLIP] > 0 and n[0, FAST] + n[0, FAST_CLIP] == trials[0]
    assert not n[0, FIRST_REJECTED:].any()
    # every first trial that was not taken as it stood ended in exactly one row-pass accept, and no row-pass accept happened without one
    for b in range(3):
        assert n[b, FIRST_REJECTED] == n[b, BACKTRACK] + n[b, CORR] + n[b, FALLBACK]
        assert n[b].sum() - n[b, FIRST_REJECTED] <= g["iters"][b]      # (entering / leaving the phase and restarts count as iterations too)
        # trial points: one per fused first trial, at least one more per back-tracked or corrected step (the correction re-tests the same point:
        # no new trial point), at least one per step of the phase unless it was a fallback step
        assert trials[b] >= n[b, FAST] + n[b, FAST_CLIP] + n[b, FIRST_REJECTED] + n[b, BACKTRACK]
    assert n[1, CORR] >= 1 and n[1, FEAS] >= 1 and n[1, FAST] >= 1
    assert n[2, BACKTRACK] >= 1 and n[2, CORR] >= 1 and n[2, FEAS] >= 1 and n[2, FAST_CLIP] >= 1
    L.close()
