"""GPU tests (MI355X, run with -m gpu) of the Newton step the kinodynamic refinement solver takes INSIDE its feasibility phase, its update and its step lengths, against
tests/elastic_newton_reference.py: the device counterpart of tests/test_kd_feas_step_cpu.py (construction and tolerances: tests/feas_step_harness.py,
tests/kd_feas_step_harness.py).  Portfolio off; the 16 drop states per horizon of tests/test_gpu_kd_step.py (batch()); members the presolve certifies are left out.

Cases: N = 2 and N = 20 with M = 12 (entry, first step, j in {1, 2, 5}); N = 2 with M = 27 (j in {12, 25}).
  * N = 2, M = 27 takes OTHER MEMBERS OF THE SAME POOL: of the first 16 drop states of batch(2), five (positions 2, 7, 8, 10, 12 of the pool's level members) converge
    or are handed back by the phase before its 26th step -- 10 of 32 pairs, more than the one in five allowed.  LATE_POSITIONS replaces them by the next positions of
    the pool whose runs stay inside the phase (found with one measuring launch over the first 35 level members: 21 stay).
  * N = 20 has no pair j = 12 or 25: every stepping member of its batch converges within 17 .. 27 iterations (member 11: 52), so with M = 27 none enters the phase, and a
    smaller M ends the phase earlier (2 M); with M = 16, j = 12, 3 of 12 stepping members are handed back first (one in four).  The batch has no other members.

Bound: 16 x max(e_aug, e_cond, 1e-15) at N = 20.  At N = 2 the measured ratio exceeds 16 on the EMULATION already: 313.118 (member 11 of batch(2), first step of the
phase, equality multipliers: an error of 1.2e-12 against yardsticks of 4e-15, normwise backward error 4.0e-18; dx 17.3, ds 7.7; run by hand through tests/emu on this
batch, 16 members x M = 12) -- the short horizon of kd_step_harness.SHORT_LATER_FACTOR, whose 300-unknown systems the sparse LU solves far below eps.  The factor there is
2 x that worst ratio, SHORT_FACTOR = 626, with the normwise backward error <= 1e-12 asserted beside it (kd_feas_step_harness.check_pair, the precedent of
kd_step_harness.check_step).

Worst measured ratio error / max(e_aug, e_cond, 1e-15) on the MI355X, dx / ds / y, pairs checked / skipped:
    N = 2,  M = 12     28.1 / 29.7 / 133      64 / 0     (bound 626; member 11, j = 0 and 1; backward error <= 1.3e-17)
    N = 20, M = 12     0.17 / 0.16 / 0.32     48 / 0     (bound 16; members 1, 7, 8, 9 certified by the presolve and left out)
    N = 2,  M = 27     5.84 / 5.82 / 16.7     32 / 0     (bound 626; j in {12, 25}, LATE_POSITIONS)
"""
import numpy as np
import pytest

import feas_step_harness as F
import kd_feas_step_harness as KF
import kd_step_harness as KH
import newton_reference as nr
import test_gpu_kd_step as T
from conftest import lc

pytestmark = pytest.mark.gpu
# (N, M, js (None: every pair M holds))
CASES = [(2, 12, None), (20, 12, None), (2, 27, [12, 25])]
SHORT_FACTOR = {2: 626.0}      # (docstring)
LATE_POSITIONS = [0, 1, 3, 4, 5, 6, 9, 11, 13, 14, 15, 16, 17, 21, 22, 24]      # (docstring: N = 2, M = 27)


@pytest.fixture(scope="module")
def ctx():
    L = lc("capi").LandingLib(20, device=0)
    R = lc("rbd").Rbd(L)
    yield L, R
    L.close()


def late_batch(N):
    """(problems, X0) of the LATE_POSITIONS of the pool batch(N) takes its first 16 from (tests/test_gpu_kd_step.py: same seed, law, grid and level test)"""
    P = lc("problem")
    consts = P.production_constants("main")
    _, X0, q, qd = P.make_batch(T.POOL, N, T.HORIZON_T(N), seed=T.SEED(N), consts=consts, dt_grid="uniform", law=T.LAW)
    pick = np.nonzero((np.abs(q[:, 3:5]) <= T.LEVEL).all(axis=1))[0][LATE_POSITIONS]
    dt = P.dt_of(N, T.HORIZON_T(N), "uniform")
    probs, x0 = zip(*[KH.problem_of(N, q[b], qd[b], X0[b], dt, consts.mu) for b in pick])
    return list(probs), np.array(x0)


@pytest.mark.parametrize("case", CASES, ids=["N%d-M%d" % c[:2] for c in CASES])
def test_gpu_phase_steps_are_newton_steps_of_the_elastic_problem(ctx, case):
    N, M, js = case
    L, R = ctx
    probs, X0 = T.batch(L, N) if M < 27 else late_batch(N)
    js = F.pairs_within(M) if js is None else js
    opts = KF.feas_opts(R, M)
    runs = {cap: KF.capped_run(R, probs, X0, opts, cap) for cap in F.caps_of(M, js)}
    res = KF.check_config(probs, opts, M, js, runs, "gpu kd N %d M %d" % (N, M), factor=SHORT_FACTOR.get(N, nr.TOL_FACTOR))
    total = res["checked"] + len(res["skipped"])
    assert len(res["members"]) >= 8 and total == len(res["members"]) * len(js) and len(res["skipped"]) * 5 <= total, res["skipped"]
