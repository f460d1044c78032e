"""The whole-body SQP kernels one at a time on the GPU: the cases of tests/test_wb_kernels_cpu.py with the product library (laws, references and checks
in tests/wb_reference.py).  Small shapes only -- every case takes a few seconds at the most, most of it the numpy references; the whole file ran in 4.2 s on an MI355X.  The figures measured on an MI355X
are in the docstrings next to the host emulation's."""
import numpy as np
import pytest

import wb_reference as wr
from conftest import GOLDEN, lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def std():
    L = lc("capi").LandingLib(20, device=0)
    yield wr.WbCalls(L, wr.CudaMem())
    L.close()


@pytest.fixture(scope="module")
def perm():
    L = lc("capi").LandingLib(20, device=0)
    yield wr.WbCalls(L, wr.CudaMem(), model=wr.permuted_model())
    L.close()


@pytest.mark.parametrize("semi", [False, True])
@pytest.mark.parametrize("N,B", [(1, 1), (3, 3), (7, 5)])
def test_backward_against_riccati_and_kkt_gpu(std, N, B, semi):
    """Bound 1e-10 relative (tests/test_wb_kernels_cpu.py states the references).  Measured, worst of the six cases, emulation | MI355X:
    K 1.9e-13 | 4.5e-14, kff 9.4e-14 | 4.5e-14, dV 4.5e-15 | 3.4e-15, du 1.8e-13 | 8.7e-14, value 1.3e-14 | 5.8e-15, dV[1] + dV[0] / 2: 0 | 0."""
    fig = wr.check_backward(std, N, B, semi)
    print("backward N=%d B=%d semi=%d:" % (N, B, semi), {k: "%.1e" % v for k, v in fig.items()})
    for k in ("K", "kff", "dV", "du", "value", "half"):
        assert fig[k] <= 1e-10, (k, fig[k])


@pytest.mark.parametrize("semi", [False, True])
def test_backward_singular_member_and_batch_independence_gpu(std, semi):
    """ok = 0 and finite outputs for the member whose Quu is not positive definite; every other member bit-identical to a call on it alone (this is also what the
    barriers around the register-held update of V protect) and equal to the oracle: emulation 3.6e-14 | MI355X 6.6e-14"""
    worst = wr.check_backward_branches(std, semi)
    print("backward branches semi=%d: %.1e" % (semi, worst))
    assert worst <= 1e-10


@pytest.mark.parametrize("nalpha,B", [(1, 1), (2, 8), (5, 7)])
@pytest.mark.parametrize("with_f,semi,closed", [(True, False, True), (False, True, True), (True, True, False), (False, False, False)])
def test_rollout_every_slot_gpu(std, with_f, semi, closed, nalpha, B):
    """1, 16 and 35 threads; with / without foot forces, explicit / semi-implicit, closed / open loop each in two of the four combinations.  Bound 1e-12 relative
    to max(1, |.|).  Measured, arrow path, worst case, emulation | MI355X: x 2.0e-15 | 3.2e-15, u 2.7e-15 | 1.8e-15, cost 7.3e-15 | 6.0e-15."""
    fig = wr.check_rollout(std, nalpha, B, 4, with_f, semi, closed)
    print("rollout arrow f=%d semi=%d closed=%d %dx%d:" % (with_f, semi, closed, nalpha, B), {k: "%.1e" % v for k, v in fig.items()})
    assert max(fig.values()) <= 1e-12, fig


@pytest.mark.parametrize("nalpha,B", [(1, 1), (2, 8), (5, 7)])
@pytest.mark.parametrize("semi,closed", [(False, True), (True, True), (False, False)])
def test_rollout_every_slot_generic_tree_gpu(perm, semi, closed, nalpha, B):
    """chol_solve18_lds and the parent-table recursion.  Measured, worst case, emulation | MI355X: x 1.0e-15 | 1.1e-15, u 1.0e-15 | 8.7e-16, cost 3.6e-15 | 3.6e-15."""
    fig = wr.check_rollout(perm, nalpha, B, 4, False, semi, closed, permuted=True)
    print("rollout dense semi=%d closed=%d %dx%d:" % (semi, closed, nalpha, B), {k: "%.1e" % v for k, v in fig.items()})
    assert max(fig.values()) <= 1e-12, fig


def test_rollout_skip_mask_is_applied_and_consumed_once_gpu(std):
    wr.check_rollout_skip(std, True)


def test_rollout_velocity_update_equals_the_dynamics_kernels_gpu(std, perm):
    """N = 1: qd+ - qd against dt qdd of landing_fb_dynamics_batch, bound 1e-12.  MI355X: arrow path 6.4e-16 (bit-equal: no), dense path 1.0e-16 (bit-equal:
    no -- the device compiler contracts the LDS copy and the private-array copy of the recursion into FMAs differently; the emulation: 6.4e-16 / no, 1.0e-16 / yes)."""
    e_arrow, bit_arrow = wr.check_rollout_header_claim(std, True)
    e_dense, bit_dense = wr.check_rollout_header_claim(perm, False)
    print("rollout vs dynamics kernels: arrow %.1e bit-equal %s, dense %.1e bit-equal %s" % (e_arrow, bit_arrow, e_dense, bit_dense))
    assert e_arrow <= 1e-12 and e_dense <= 1e-12


@pytest.mark.parametrize("nalpha", [1, 4])
@pytest.mark.parametrize("N", [3, 8])
def test_select_against_numpy_restatement_gpu(std, N, nalpha):
    wr.check_select(std, N, nalpha)


def test_select_argument_errors_gpu(std):
    wr.check_select_argument_errors(std)


@pytest.mark.parametrize("name,semi,fused", [("a", False, True), ("b", False, True), ("mixed", False, True), ("a", True, True), ("mixed", False, False)])
def test_loop_backtracks_like_the_oracle_gpu(name, semi, fused):
    """N = 5, B = 6, 3 iterations on lists whose first entry overshoots, against the oracle's record (tests/golden/wb_backtrack.npz, which the CPU test holds equal to
    the oracle): every member's alphas, the cost history to 1e-9 relative (emulation 2.7e-12 | MI355X 2.7e-12).  "mixed": member 5 takes the first entry, the others
    the second in stage 2 of the fused search; the host loop (fused = False) gives the same alphas and costs to rounding."""
    alphas = wr.LOOP_LISTS[name]
    L = lc("capi").LandingLib(20, device=0)
    out = wr.loop_run(L, "cuda", alphas, semi, fused)
    al, hist = wr.loop_golden(GOLDEN, name, semi)
    print(name, semi, fused, out["alpha"].tolist(), "cost history vs oracle %.1e" % np.max(np.abs(out["cost"] - hist) / hist))
    assert np.array_equal(out["alpha"], al), (out["alpha"], al)
    assert np.max(np.abs(out["cost"] - hist) / hist) <= 1e-9
    if name == "mixed" and fused:
        host = wr.loop_run(L, "cuda", alphas, semi, False)
        for k in ("alpha", "cost", "x", "u"):
            assert np.array_equal(out[k], host[k]), k
    L.close()


def test_generic_tree_dynamics_against_oracle_and_quad_path_gpu(perm, std):
    """npts = 70: one full workgroup of 64 and a ragged one for the per-point kernels, 2 520 threads for the tangent kernel.  H, C, qdd, Hinv and the quad path's A at
    every point, the oracle's Richardson and central-difference Jacobians at the first 3.  Bounds of tests/test_rbd.py, 1e-12 for A against the quad path.  Measured,
    emulation (3 points) | MI355X (70 points, other draws): H 2.2e-16 | 6.5e-16, C 1.3e-16 | 5.3e-16, qdd 9.2e-16 | 3.7e-14, Hinv 9.9e-16 | 1.2e-13, exact A vs Richardson 9.8e-10 | 2.0e-11,
    central-difference A 7.1e-9 | 2.3e-9, exact A vs quad path 2.2e-15 | 4.4e-15."""
    fig = wr.check_generic_tree(perm, std, 70, 3)
    print("generic tree:", {k: "%.1e" % v for k, v in fig.items()})
    for k, bound in wr.GENERIC_BOUNDS.items():
        assert fig[k] <= bound, (k, fig[k])
