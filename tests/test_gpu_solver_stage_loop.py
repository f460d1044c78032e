"""GPU test (MI355X): the two instances of the backward sweep's stage loop agree, and the sweep counters add up.

riccati_backward runs the stages N - 2 .. 0 in one resident loop; the instance that reads the clock around every stage is chosen once per
sweep when the profile buffer is set, the other carries no trace of the timers.  Both must compute the same: x, f, lam_g, status, iters
and kkt of a solve with the profile buffer set and of one with it unset are np.array_equal.  Shapes: B = 16 at N = 2 (the last stage plus
ONE trip of the loop), N = 3 and N = 6, and B = 8 at N = 40 (the benchmark's horizon), iteration limit 12, feasibility phase off (so that
`iters` counts the steps of the one interior-point loop).

Counters of the profile buffer, per member, with S sweeps started, A stage eliminations attempted and K succeeded (the foot block of stage
0 counts as one: a complete sweep is N + 1 eliminations):
  * A - K is the number of abandoned sweeps, which is S minus the steps taken (`iters`): every iteration that computes a step has exactly
    one complete sweep; at N = 2 the members do abandon sweeps, which is asserted, so the identity is not 0 = 0;
  * K = (N + 1) (S - F) + what the F abandoned sweeps got through before their failing elimination, between 0 and N each."""
import numpy as np
import pytest

from conftest import lc

pytestmark = pytest.mark.gpu

KEYS = ("x", "f", "lam_g", "status", "iters", "kkt")
PH_NFACT, PH_NSTAGE_OK, PH_NSTAGE = 8, 11, 13


@pytest.mark.parametrize("N,B", [(2, 16), (3, 16), (6, 16), (40, 8)])
def test_timed_and_untimed_stage_loop_agree(N, B):
    import torch
    capi, problem = lc("capi"), lc("problem")
    L = capi.LandingLib(N, device=0)
    P, X0, _, _ = problem.make_batch(B, N, 0.6, seed=20211)
    o = L.default_opts()
    o.max_iter = 12
    o.feas_phase = 0
    plain = {k: np.asarray(v).copy() for k, v in L.solve_host(P, X0, o).items()}
    prof = torch.zeros(B, 16, device="cuda", dtype=torch.float64)
    L.lib.landing_set_profile_buffer(L.ctx, prof.data_ptr())
    timed = {k: np.asarray(v).copy() for k, v in L.solve_host(P, X0, o).items()}
    L.lib.landing_set_profile_buffer(L.ctx, None)
    ph = prof.cpu().numpy()
    L.close()
    S, A, K = (ph[:, i].astype(np.int64) for i in (PH_NFACT, PH_NSTAGE, PH_NSTAGE_OK))
    F = A - K
    it, st = timed["iters"].astype(np.int64), timed["status"]
    print("N", N, "status", st.tolist(), "iters", it.tolist(), "sweeps", S.tolist(), "attempted", A.tolist(), "ok", K.tolist())
    for k in KEYS:
        assert np.array_equal(plain[k], timed[k]), "%s differs between the untimed and the timed stage loop" % k
    assert (S > 0).all() and (A >= S).all()
    # steps taken: every counted iteration computed a step from exactly one complete sweep (an iteration that ends the solve for want of a
    # factorisation is not counted in `iters`; the emulation shows the same for the N = 2 members, which end that way)
    print("abandoned", F.tolist(), "sweeps - iters", (S - it).tolist())
    assert np.array_equal(F, S - it), "attempted - ok is not the number of abandoned sweeps (sweeps started - steps taken)"
    if N == 2:      # these members abandon sweeps (60 each within 16 iterations in the emulation): the check above is not 0 == 0
        assert F.sum() > 0, "no member abandoned a sweep"
    rest = K - (N + 1) * (S - F)
    assert ((rest >= 0) & (rest <= N * F)).all(), "ok is not (N + 1) per complete sweep + the partial counts of the abandoned ones"
