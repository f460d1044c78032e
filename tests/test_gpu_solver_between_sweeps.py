"""GPU test (MI355X): the phases between the two sweeps after their memory accesses were rearranged -- same steps, same bits.

The derivative phase of landing_ipm_kernel reads the multipliers from a copy in LDS (stage k at 36 + 105 k, laid over [G | P | A1 | A^]) at
horizons up to 44 and from the workspace beyond.  The host emulation runs the same index arithmetic but knows no address spaces and no
`ds_read`; whether the device reads the slot that was written shows here.  8 members at N = 2, 3, 5, 6 (the copy's 80-row last stage one
to five strides behind the boundary rows), N = 40 (the benchmark's horizon) and N = 44 / 45 (both sides of the copy's limit):

  * the step.  dx, ds, yn of the first iteration at every horizon, and of iteration 5 at N = 40, against the independent Newton-system solve
    of tests/newton_reference.py (tests/solver_step_harness.py, the bound of tests/test_gpu_solver_step.py: per quantity
    16 x max(e_aug, e_cond, 1e-15), unchanged).  A multiplier read from the wrong slot gives another grad f + J^T y and another Hessian, hence
    another step.  (The first step starts from y = z_U - z_L, y_dyn = 0: the bound multipliers are 1 there, so the J^T y sums and the Hessian's
    inequality terms are not trivial.)
  * full solves, default options: x, f, lam_g, iters, status, kkt are np.array_equal to tests/golden/between_sweeps_gpu.npz (N = 44, 45:
    between_sweeps_gpu_long.npz), recorded on the MI355X from the product library of the commit BEFORE the change
    (tests/make_golden_between_sweeps.py --gpu).  Bit-equality is the claim: no tolerance.
"""
import numpy as np
import pytest

import make_golden_between_sweeps as rec
import solver_step_harness as H
from conftest import lc

pytestmark = pytest.mark.gpu

HORIZONS = [2, 3, 5, 6, 40, 44, 45]
B = 8
LATER_K = 4      # the step of iteration LATER_K + 1 from the state run LATER_K ended in


def batch(N):
    return lc("problem").make_batch(B, N, 0.6, seed=500 + N)[:2]


@pytest.fixture(scope="module")
def golden():
    parts = {part: np.load(path) for part, path in rec.GPU_GOLDEN.items()}
    return {N: parts[part] for part, horizons in rec.GPU_HORIZONS.items() for N in horizons}


@pytest.mark.parametrize("N", HORIZONS)
def test_gpu_between_sweeps_first_step_is_the_newton_step(oracle_mod, N):
    O = oracle_mod.Oracle(N)
    L = lc("capi").LandingLib(N, device=0)
    P, X0 = batch(N)
    w, nfact, _ = H.first_step_group(L, O, P, X0, H.step_opts(L, (1e-2, 0.1), 1), "gpu between sweeps first N %d" % N, plain_form=True)
    L.close()
    print("gpu between sweeps N %d: first step worst ratio %.3g (factorisations max %d)" % (N, w, nfact.max()))


def test_gpu_between_sweeps_later_step_is_the_newton_step(oracle_mod):
    N = 40
    O = oracle_mod.Oracle(N)
    L = lc("capi").LandingLib(N, device=0)
    P, X0 = batch(N)
    runs = {K: H.kernel_run(L, P, X0, H.step_opts(L, None, K)) for K in (LATER_K, LATER_K + 1)}
    w, n, skipped = H.later_step_pairs(runs, O, P, "gpu between sweeps later N %d" % N)
    L.close()
    print("gpu between sweeps N %d, step %d: %d checked, %d skipped, worst ratio %.3g" % (N, LATER_K + 1, n, len(skipped), w))
    for s in skipped:
        print("  skipped:", s)
    assert n + len(skipped) == B and n >= B // 2, "fewer than half of the members reached a checked step %d" % (LATER_K + 1)


@pytest.mark.parametrize("N", HORIZONS)
def test_gpu_between_sweeps_full_solves_equal_the_parent_bit_for_bit(golden, N):
    assert sorted(sum(rec.GPU_HORIZONS.values(), ())) == HORIZONS and rec.GPU_B == B
    out = rec.gpu_solve(N)
    print("N", N, "status", out["status"].tolist(), "iters", out["iters"].tolist())
    assert (out["iters"] >= 1).all()
    for k in rec.KEYS:
        want = golden[N]["n%d_%s" % (N, k)]
        assert out[k].shape == want.shape and out[k].shape[0] == B, k
        for m in range(B):      # every member, every field
            assert np.array_equal(out[k][m], want[m]),"N %d: %s of member %d differs from the parent build's" % (N, k, m)
