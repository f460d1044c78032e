"""GPU tests (MI355X) of the Newton step landing_ipm_kernel computes, against tests/newton_reference.py: the device counterpart of
tests/test_solver_step_cpu.py (read its docstring for the construction, the bound and the regularisation convention).  The device differs
from the host emulation in the reciprocal (v_rcp_f64 + two Newton steps) and in the accumulation order of the fp64 matrix cores.

Batches of 64 members per launch at N = 20, 40, 80, 96, every member checked -- which also covers the per-member stride of the workspace --
and one batch of 576 members, which goes through the hard-first dispatch order (order[], batches above 512).

Bound: per quantity, error <= 16 x max(e_aug, e_cond, 1e-15).  Worst measured ratio error / max(e_aug, e_cond, 1e-15) on the MI355X:
    first step    5.8   (N = 20, bound_push = mu_init = 1e-6, equality multipliers; 3.4 .. 4.1 at N = 40, 80, 96; dx / ds stay below 0.1;
                         running-cost form and production grid 0.68, the 576-member launch 0.13)
    later steps   7.4   (N = 20, K = 5, equality multipliers; dx <= 2.2, ds <= 3.0; N = 40 / 80 / 96: 3.0 / 7.1 / 3.9); 1275 pairs checked,
                         5 skipped (N = 20, K = 25: members that had converged before iteration 26), no restart met
(host emulation: 2.0 and 0.32).  Normwise backward error of the kernel's step, printed per member with -s: <= 1.6e-13.
NOT caught by these tests: fast_rcp cut to ONE Newton step in a scratch device build (first step, N = 20: worst ratio 5.0, passes) -- one
step leaves the reciprocal within a few ulp, which is rounding level for this bound.
"""
import pytest

import solver_step_harness as H
from conftest import lc

pytestmark = pytest.mark.gpu
SEED = lambda N: 300 + N
# (option set, delta_floor) of the first-step launches at every horizon
FIRST_LAUNCHES = [((1e-2, 0.1), None), ((1e-4, 1e-2), 0.0), ((1e-6, 1e-6), None), ((1e-8, 1e-4), 0.0), ("warm", None)]


@pytest.fixture(scope="module")
def oracle_cls(oracle_mod):
    return oracle_mod.Oracle


@pytest.mark.parametrize("N", [20, 40, 80, 96])
def test_gpu_first_step_is_the_newton_step(oracle_cls, N):
    B = 64
    O = oracle_cls(N)
    L = lc("capi").LandingLib(N, device=0)
    P, X0, _, _ = lc("problem").make_batch(B, N, 0.6, seed=SEED(N))
    worst = 0.0
    for oset, floor in FIRST_LAUNCHES:
        name = "gpu first N %d opts %s floor %s" % (N, oset, floor)
        w, nfact, _ = H.first_step_group(L, O, P, X0, H.step_opts(L, oset, 1, floor), name, plain_form=True)
        worst = max(worst, w)
        print("%s: worst ratio %.3g, factorisations max %d" % (name, w, nfact.max()))
    print("gpu first step N %d: WORST RATIO %.3g" % (N, worst))
    L.close()


def test_gpu_first_step_running_cost_and_production_grid(oracle_cls):
    """the running-cost form (proximal floor 0) at N = 40 and the reference's production grid with the data-generation law at N = 20"""
    Pm = lc("problem")
    O = oracle_cls(40, run_cost=H.RUN_COST)
    L = lc("capi").LandingLib(40, device=0, run_cost=H.RUN_COST)
    P, X0, _, _ = Pm.make_batch(64, 40, 0.6, seed=11)
    w1, _, _ = H.first_step_group(L, O, P, X0, H.step_opts(L, None, 1), "gpu first rc N 40 auto", plain_form=False)
    L.close()
    O = oracle_cls(20)
    L = lc("capi").LandingLib(20, device=0)
    P, X0, _, _ = Pm.make_batch(64, 20, 0.6, seed=100000, consts=Pm.production_constants("datagen"), dt_grid="reference", law="datagen")
    w2, _, _ = H.first_step_group(L, O, P, X0, H.step_opts(L, (1e-4, 1e-2), 1), "gpu first production grid", plain_form=True)
    print("gpu first step forms / grid: WORST RATIO %.3g" % max(w1, w2))
    L.close()


def test_gpu_first_step_hard_first_dispatch_order(oracle_cls):
    """576 members: above 512 the launch runs the members in the order of landing_order_kernel; every member's block must still hold its own step"""
    N, B = 20, 576
    O = oracle_cls(N)
    L = lc("capi").LandingLib(N, device=0)
    o = H.step_opts(L, (1e-2, 0.1), 1)
    assert o.dispatch_order == 1
    P, X0, _, _ = lc("problem").make_batch(B, N, 0.6, seed=77)
    w, _, _ = H.first_step_group(L, O, P, X0, o, "gpu first order[] B 576", plain_form=True)
    print("gpu first step order[]: WORST RATIO %.3g" % w)
    L.close()


@pytest.mark.parametrize("N", [20, 40, 80, 96])
def test_gpu_later_steps_are_newton_steps(oracle_cls, N):
    """K in {1, 2, 5, 12, 25}, 64 members: state from run K, step from run K + 1 (tests/test_solver_step_cpu.py).  Skipped: members that
    converged before iteration K + 1 and iterations without a factorisation (restart); at most one pair in five."""
    B = 64
    O = oracle_cls(N)
    L = lc("capi").LandingLib(N, device=0)
    P, X0, _, _ = lc("problem").make_batch(B, N, 0.6, seed=SEED(N))
    Ks = sorted(set(H.LATER_K) | {k + 1 for k in H.LATER_K})
    runs = {K: H.kernel_run(L, P, X0, H.step_opts(L, None, K)) for K in Ks}
    worst, n, skipped = H.later_step_pairs(runs, O, P, "gpu later N %d" % N)
    print("gpu later steps N %d: %d pairs checked, %d skipped, WORST RATIO %.3g" % (N, n, len(skipped), worst))
    for s in skipped:
        print("  skipped:", s)
    assert n + len(skipped) == B * len(H.LATER_K) and len(skipped) * 5 <= n + len(skipped)
    L.close()
