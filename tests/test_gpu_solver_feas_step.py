"""GPU tests (MI355X, run with -m gpu) of the Newton step landing_ipm_kernel takes INSIDE its feasibility phase, its update and its step lengths, against
tests/elastic_newton_reference.py: the device counterpart of tests/test_solver_feas_step_cpu.py (read its docstring and tests/feas_step_harness.py for the construction,
the iteration cap, the pairs a run with max_iter = M can hold, and the tolerances).  The device differs from the host emulation in its divisions (reciprocal plus
Newton steps) and in the accumulation order of the fp64 matrix cores.

Launches of at most 16 members and at most 54 iterations; the reference solves run on the host in the harness's thread pool (solver_step_harness.REF_THREADS).

Worst measured ratio error / max(e_aug, e_cond, 1e-15) on the MI355X (bound 16), dx / ds / y, pairs checked / skipped:
    named N = 20, rho 1000, M = 2     0.080   / 0.080   / 0.022      16 / 0
    named N = 20, rho 1000, M = 12    0.060   / 0.16    / 0.015      64 / 0
    named N = 20, rho 1000, M = 27    0.048   / 0.023   / 0.12       27 / 5    all twelve locally infeasible members checked at j = 25
    named N = 20, rho 10,   M = 2     0.078   / 0.078   / 0.052      16 / 0
    named N = 20, rho 10,   M = 12    0.31    / 0.89    / 0.32       64 / 0
    running cost N = 40,    M = 2     0.044   / 0.044   / 0.0093     16 / 0
    running cost N = 40,    M = 12    0.020   / 0.020   / 0.017      64 / 0
    N = 96,                 M = 12    0.00044 / 0.00044 / 0.00040    23 / 1
(host emulation: tests/test_solver_feas_step_cpu.py; the two agree in size.)  Normwise backward error of the kernel's step, printed per pair with -s: <= 3.0e-17.
Skipped pairs: named rho 1000 M = 27 -- converging member (100000, 0) at j = 12 (handed back by the phase: feas = 0) and at j = 25 (status 0 after 48 iterations), converging
members (100000, 1), (100000, 2), (100000, 3) at j = 25 (handed back); N = 96 member 1 at j = 5 (handed back exactly at the cap: 20 iterations counted, no step taken).
Measured once and NOT a committed case: named rho 10 M = 27 -- 9 pairs checked, 23 of 32 skipped (the phase hands the members back), worst 5.9 / 6.0 / 5.8.
"""
import pytest

import feas_step_harness as F
import solver_step_harness as H
from conftest import lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle_cls(oracle_mod):
    return oracle_mod.Oracle


def _config(L, O, P, X0, M, js, label, rho=None):
    opts = F.feas_opts(L, M, rho)
    runs = {cap: F.capped_run(L, P, X0, opts, cap) for cap in F.caps_of(M, js)}
    res = F.check_config(O, P, opts, M, js, runs, label)
    total = res["checked"] + len(res["skipped"])
    assert total == P.shape[0] * len(js) and len(res["skipped"]) * 5 <= total, (label, res["skipped"])
    return res


@pytest.mark.parametrize("rho", [1000.0, 10.0])
def test_gpu_phase_steps_of_the_named_members(oracle_cls, rho):
    """N = 20 production grid, the 12 + 4 named members in ONE batch of 16, M in {2, 12}: entry state, first step and the pairs j in {1, 2, 5}; at rho = 1000 also
    M = 27 with the pairs j in {12, 25}, where at least six of the twelve locally infeasible members contribute a checked pair at j = 25.  (At rho = 10 the phase hands
    most members back before its 25th step -- 23 of 32 pairs at M = 27 have no step inside it -- so the cheap price keeps to M in {2, 12}.)"""
    N = 20
    O = oracle_cls(N)
    P, X0 = F.named_batch(N)
    L = lc("capi").LandingLib(N, device=0)
    out = {M: _config(L, O, P, X0, M, F.pairs_within(M) if M < 27 else [12, 25], "gpu named rho %g M %d" % (rho, M), rho) for M in ((2, 12, 27) if rho == 1000.0 else (2, 12))}
    L.close()
    if rho == 1000.0:
        assert len([b for b in out[27]["by_j"][25] if b < 12]) >= 6, out[27]["by_j"]


def test_gpu_phase_steps_of_the_running_cost_form(oracle_cls):
    """N = 40, running-cost form, 16 members, M in {2, 12}"""
    N = 40
    O = oracle_cls(N, run_cost=H.RUN_COST)
    P, X0, _, _ = lc("problem").make_batch(16, N, 0.6, seed=20211)
    L = lc("capi").LandingLib(N, device=0, run_cost=H.RUN_COST)
    for M in (2, 12):
        _config(L, O, P, X0, M, F.pairs_within(M), "gpu rc N 40 M %d" % M)
    L.close()


def test_gpu_phase_steps_at_the_longest_horizon(oracle_cls):
    """N = 96, 8 members, M = 12, j in {0, 1, 5}"""
    N = 96
    O = oracle_cls(N)
    P, X0, _, _ = lc("problem").make_batch(8, N, 0.6, seed=300 + N)
    L = lc("capi").LandingLib(N, device=0)
    _config(L, O, P, X0, 12, [0, 1, 5], "gpu N 96 M 12")
    L.close()
