"""GPU test (MI355X): the forward recursion's 8-lane sums travel by DPP on the device -- are they still sums?

On the device forward_pass adds the partial products of a row with quad_perm / row_shl moves inside the vector ALU (lane_sum8_head), and
the assembly hooks of the backward sweep carry their term words across a block step.  The host emulation keeps __shfl_xor, so only the
device shows whether the DPP controls pick the partners the butterfly picked.  Two checks, 8 members at N = 2, 3, 5, 6 (no multiples of the forward loop's unroll factor 4: clamped prefetches, `k < N` guards)
and N = 40 (the benchmark's horizon), through the existing entry points:

  * the step.  dx, ds, yn of the first iteration at every horizon, and of iteration 5 at N = 40, against the independent Newton-system solve
    of tests/newton_reference.py (tests/solver_step_harness.py, the bound of tests/test_gpu_solver_step.py: per quantity
    16 x max(e_aug, e_cond, 1e-15), unchanged).  A wrong partner in the 8-lane sum gives a state recursion that is no solution of that
    system; a term word that did not survive the block step gives another G, gamma or A^ and so another step.  Later steps are held to the bound at N = 40 only: by iteration 5 the members of the short
    horizons run with delta_w up to 0.61, where the bound (two unrefined LU solves of the same system) is no yardstick any more -- the host
    emulation, whose arithmetic this change leaves bit-identical to the parent's, misses it at N = 2 (ratio 21 on dx, 34 on y, members 5 and 7).
  * the two instances of the backward loop.  x, f, lam_g, status, iters and kkt of a 12-iteration solve with the profile buffer set (timed)
    and unset are np.array_equal.
"""
import numpy as np
import pytest

import solver_step_harness as H
from conftest import lc

pytestmark = pytest.mark.gpu

HORIZONS = [2, 3, 5, 6, 40]
B = 8
KEYS = ("x", "f", "lam_g", "status", "iters", "kkt")
LATER_K = 4      # the step of iteration LATER_K + 1 from the state run LATER_K ended in


def batch(N):
    return lc("problem").make_batch(B, N, 0.6, seed=500 + N)[:2]


@pytest.mark.parametrize("N", HORIZONS)
def test_gpu_forward_chain_first_step_is_the_newton_step(oracle_mod, N):
    O = oracle_mod.Oracle(N)
    L = lc("capi").LandingLib(N, device=0)
    P, X0 = batch(N)
    w, nfact, _ = H.first_step_group(L, O, P, X0, H.step_opts(L, (1e-2, 0.1), 1), "gpu forward chain first N %d" % N, plain_form=True)
    L.close()
    print("gpu forward chain N %d: first step worst ratio %.3g (factorisations max %d)" % (N, w, nfact.max()))


def test_gpu_forward_chain_later_step_is_the_newton_step(oracle_mod):
    N = 40
    O = oracle_mod.Oracle(N)
    L = lc("capi").LandingLib(N, device=0)
    P, X0 = batch(N)
    runs = {K: H.kernel_run(L, P, X0, H.step_opts(L, None, K)) for K in (LATER_K, LATER_K + 1)}
    w, n, skipped = H.later_step_pairs(runs, O, P, "gpu forward chain later N %d" % N)
    L.close()
    print("gpu forward chain N %d, step %d: %d checked, %d skipped, worst ratio %.3g" % (N, LATER_K + 1, n, len(skipped), w))
    for s in skipped:
        print("  skipped:", s)
    assert n + len(skipped) == B and n >= B // 2, "fewer than half of the members reached a checked step %d" % (LATER_K + 1)


@pytest.mark.parametrize("N", HORIZONS)
def test_gpu_forward_chain_timed_and_untimed_agree(N):
    import torch
    L = lc("capi").LandingLib(N, device=0)
    P, X0 = batch(N)
    o = L.default_opts()
    o.max_iter = 12
    o.feas_phase = 0
    plain = {k: np.asarray(v).copy() for k, v in L.solve_host(P, X0, o).items()}
    prof = torch.zeros(B, 16, device="cuda", dtype=torch.float64)
    L.lib.landing_set_profile_buffer(L.ctx, prof.data_ptr())
    timed = {k: np.asarray(v).copy() for k, v in L.solve_host(P, X0, o).items()}
    L.lib.landing_set_profile_buffer(L.ctx, None)
    L.close()
    print("N", N, "status", timed["status"].tolist(), "iters", timed["iters"].tolist())
    assert (timed["iters"] >= 1).all()
    for k in KEYS:
        assert np.array_equal(plain[k], timed[k]), "%s differs between the untimed and the timed build of the sweeps" % k
