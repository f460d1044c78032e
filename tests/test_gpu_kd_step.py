"""GPU tests (MI355X) of the Newton step the kinodynamic refinement solver computes, against tests/kd_newton_reference.py: the device counterpart of
tests/test_kd_step_cpu.py (read its docstring for the construction, the intermediates, the bound and the regularisation convention).  The device differs from the
host emulation in the reciprocal of the pivots (v_rcp_f64 + two Newton steps), in the accumulation order of the fp64 matrix cores and in fused multiply-adds.

N in {2, 3, 20, 33, 64}, 16 members per launch, every member checked; members the presolve certifies as infeasible have no step (counted: at least 8 of a launch
step).  N = 20 runs on the production grid from the SRBM SOLUTION as the callers do, the other horizons on a uniform grid from the SRBM initial guess of
make_batch(consts = production_constants("main")) -- at N = 2 and 3 on a 50 ms grid and with the first 16 members of a 1024-member pool whose roll and pitch lie
inside the terminal box (see POOL below: tilted drop states are NOT step-checked at the short horizons).  N = 64 is where the gathered steps dxa[N][72] and dsg[24 * 65] of the forward sweep run on into Pm, pv, Ah, Y.
J and H of the reference are the function layer's (landing_kinodyn_nlp_eval / _hess); J is held against the oracle's complex-step Jacobian to 1e-11 on one member
per horizon.

Bound: per quantity, error <= 16 x max(e_aug, e_cond, 1e-15).  Worst measured ratio error / max(e_aug, e_cond, 1e-15) on the MI355X:
    first step    N = 2: 7.6    N = 3: 2.8    N = 20: 3.9    N = 33: 2.5    N = 64: 2.3     (five launches per horizon, 12 .. 16 stepping members each: 380 steps;
                  every one needs ONE factorisation; backward error <= 2.7e-12 at N = 20, <= 2.6e-13 elsewhere)
    later steps   N = 20: 0.54    N = 33: 0.19    N = 64: 0.075     (bound 16; 176 pairs, none skipped; backward error <= 8.9e-14)
                  N = 2: 2.5e3 (K = 12)    N = 3: 152     (64 pairs each, none skipped; backward error <= 2.2e-14 / 5.2e-13)
Later steps of the two short horizons exceed 16 -- on the emulation as well (360 / 170 when this file is run through the emulation, which no committed test does).  It was
treated as a finding: in every offending pair the backward error of the kernel's step is <= 5.2e-13 and Sigma, rho, gc are inside their bounds, so the matrix is right and
the forward error amplified; the sparse LU solves these 300 .. 400-unknown systems to ~1e-19.  Their factor is kd_step_harness.SHORT_LATER_FACTOR = {2: 8192, 3: 512}
(per horizon the next power of two above twice the worst ratio of emulation and device) with the backward error <= 1e-12 asserted alongside; every other case keeps 16.
gc: worst 4.7 eps of the term sums (bound min(8 eps, (n + 2) 2^-53)); product Jacobian against the complex step <= 4.4e-16.
Iterations with 3 .. 5 factorisations (the resumed inertia correction) occur among the later steps at N = 2, 3, 20, 33; that is printed, not asserted -- the path is
asserted on the CPU (tests/test_kd_step_cpu.py).
"""
import numpy as np
import pytest

import kd_step_harness as H
from conftest import lc

pytestmark = pytest.mark.gpu
B = 16
HORIZONS = (2, 3, 20, 33, 64)
LATER_K = (1, 2, 5, 12)
SEED = lambda N: 500 + N
LAW = "main"
# N = 2, 3: a drop state whose roll / pitch lies outside the terminal box (0.1 rad) cannot be brought into it in two or three intervals -- the attitude of X_1 is fixed by
# the initial rates.  Such a member jams from the fifth iteration on (steps of 1e-6, Sigma ~ 1e13), and its Newton system has no reference: neither the fp64 LU nor a dense
# LU in np.longdouble refines it to 1e-13, the residual floor being eps |K| |z| / |b|.  The short horizons therefore take the first 16 members of a pool of make_batch() drop
# states whose roll and pitch are inside the terminal box.
POOL, LEVEL = 1024, 0.1
HORIZON_T = lambda N: 0.6 if N >= 20 else 0.05 * N      # (short horizons: the 50 ms grid of the CPU tests -- two intervals of 0.3 s pose a problem whose slacks collapse, and no
                                                        # fp64 LU refines a system with Sigma ~ 1e13 to the 1e-13 the reference has to reach)
# (option set, delta_floor) of the first-step launches at every horizon
FIRST_LAUNCHES = [((1e-2, 0.1), None), ((1e-4, 1e-2), 0.0), ((1e-6, 1e-6), None), ((1e-8, 1e-4), 0.0), ("warm", None)]


@pytest.fixture(scope="module")
def ctx():
    L = lc("capi").LandingLib(20, device=0)
    R = lc("rbd").Rbd(L)
    yield L, R
    L.close()


_BATCH = {}


def batch(L, N):
    """(problems, X0) of the 16 drop states of horizon N"""
    if N not in _BATCH:
        P = lc("problem")
        consts = P.production_constants("main")
        grid = "reference" if N == 20 else "uniform"
        Pp, X0, q, qd = P.make_batch(B if N >= 20 else POOL, N, HORIZON_T(N), seed=SEED(N), consts=consts, dt_grid=grid, law=LAW)
        if N < 20:      # the first 16 drop states of the pool that are solvable in so few intervals (LEVEL)
            pick = np.nonzero((np.abs(q[:, 3:5]) <= LEVEL).all(axis=1))[0][:B]
            assert len(pick) == B, len(pick)
            Pp, X0, q, qd = Pp[pick], X0[pick], q[pick], qd[pick]
        guess = X0
        if N == 20:      # the SRBM solution, as the production callers pass it on
            srbm = L.solve_host(Pp, X0)
            assert (srbm["status"] == 0).sum() >= B - 1, srbm["status"]
            guess = srbm["x"]
        dt = P.dt_of(N, HORIZON_T(N), grid)
        probs, x0 = zip(*[H.problem_of(N, q[b], qd[b], guess[b], dt, consts.mu) for b in range(B)])
        _BATCH[N] = (list(probs), np.array(x0))
    return _BATCH[N]


def stepping(run0):
    """members with a step: all but those the presolve certifies as infeasible (status 3, no iteration)"""
    st, it = run0["res"]["status"], run0["res"]["iters"]
    members = [b for b in range(B) if not (st[b] == 3 and it[b] == 0)]
    assert len(members) >= 8, ("too few stepping members", st)
    return members


@pytest.mark.parametrize("N", HORIZONS)
def test_gpu_first_step_is_the_newton_step(ctx, N):
    L, R = ctx
    probs, X0 = batch(L, N)
    worst, worst_b, jac_checked = 0.0, 0.0, False
    for oset, floor in FIRST_LAUNCHES:
        name = "gpu first N %d opts %s floor %s" % (N, oset, floor)
        opts = H.step_opts(R, oset, 1, floor)
        runs = {K: H.kd_run(R, probs, X0, H.step_opts(R, oset, K, floor)) for K in (0, 1)}
        members = stepping(runs[0])
        jc = None if jac_checked else members[0]
        jac_checked = True

        def one(b):
            _, rec = H.member_view(runs[1], b)
            assert rec["it"] == 1 and rec["delta"] == H.nr.delta_schedule(opts, int(rec["nfact"]), opts.delta_floor), (name, b, rec)
            skip, w, bwd = H.check_pair(probs[b], X0[b], runs, 0, b, "%s member %d" % (name, b), jac="product", jac_check=(b == jc), opts=opts)
            assert skip is None, skip
            return w, bwd
        out = H.pool_map(one, members)
        w = max(o[0] for o in out); worst = max(worst, w); worst_b = max(worst_b, max(o[1] for o in out))
        print("%s: %d stepping members, worst ratio %.3g, factorisations max %d" % (name, len(members), w, max(int(H.member_view(runs[1], b)[1]["nfact"]) for b in members)))
    print("gpu first step N %d: WORST RATIO %.3g, backward error %.1e, gc %.2f eps of the term sums" % (N, worst, worst_b, H.WORST_GC[0]))


@pytest.mark.parametrize("N", HORIZONS)
def test_gpu_later_steps_are_newton_steps(ctx, N):
    """K in {1, 2, 5, 12}: state from run K, step from run K + 1 (tests/test_kd_step_cpu.py).  Skipped: members that stopped before iteration K + 1 and pairs with a
    restart between the two runs; at most one pair in five."""
    L, R = ctx
    probs, X0 = batch(L, N)
    Ks = sorted(set(LATER_K) | {k + 1 for k in LATER_K})
    runs = {K: H.kd_run(R, probs, X0, H.step_opts(R, None, K)) for K in Ks}
    members = stepping(runs[Ks[0]])
    jobs = [(K, b) for K in LATER_K for b in members]
    out = H.pool_map(lambda j: H.check_pair(probs[j[1]], X0[j[1]], runs, j[0], j[1], "gpu later N %d K %d member %d" % (N, j[0], j[1]), jac="product",
                                              factor=H.SHORT_LATER_FACTOR.get(N, H.nr.TOL_FACTOR)), jobs)
    skipped = [s for s, _, _ in out if s]
    ratios = [w for s, w, _ in out if not s]
    nf = max(int(H.member_view(runs[K + 1], b)[1]["nfact"] - H.member_view(runs[K], b)[1]["nfact"]) for K, b in jobs)
    print("gpu later steps N %d: %d pairs checked, %d skipped, WORST RATIO %.3g, backward error %.1e, most factorisations in one iteration %d, gc %.2f eps" % (
        N, len(ratios), len(skipped), max(ratios), max(b for s, _, b in out if not s), nf, H.WORST_GC[0]))
    for s in skipped:
        print("  skipped:", s)
    assert len(ratios) + len(skipped) == len(jobs) and len(skipped) * 5 <= len(jobs)
