"""The whole-body SQP kernels one at a time, on every branch, through the host emulation (tests/emu): landing_wb_backward against a dense Riccati recursion
and against one KKT solve of the LQ subproblem; landing_wb_rollout per (step length, member) against oracle/wb_oracle.py, with its skip mask;
landing_wb_select against a numpy restatement of its rule; the loop of landing-controller_amd/wb.py on step-length lists with which it really
backtracks; the generic-tree path of landing_fb_dynamics_batch / landing_wb_rollout on a renumbered quadruped; and the refusal of foot forces on a
tree whose legs are not numbered the way the foot code composes them.  Laws, references and checks: tests/wb_reference.py (shared with
tests/test_gpu_wb_kernels.py, which states the figures measured on the GPU)."""
import numpy as np
import pytest

import wb_reference as wr
from conftest import GOLDEN, lc
from emu_support import emu_landing_lib


def _lib():
    return emu_landing_lib(20)


@pytest.fixture(scope="module")
def std():
    return wr.WbCalls(_lib(), wr.HostMem())


@pytest.fixture(scope="module")
def perm():
    return wr.WbCalls(_lib(), wr.HostMem(), model=wr.permuted_model())


# ---- 1. landing_wb_backward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semi", [False, True])
@pytest.mark.parametrize("N,B", [(1, 1), (3, 3), (7, 5)])
def test_backward_against_riccati_and_kkt(std, N, B, semi):
    """K, kff, dV against the oracle's Riccati recursion on the same stage matrices; the policy rolled out linearly against du* of the dense KKT solve;
    dV[0] + dV[1] against the optimal value of the quadratic model; dV[1] = -dV[0] / 2.  Bound 1e-10 relative.  Measured (generator seed 0, worst of
    the six cases): K 1.9e-13, kff 9.4e-14, dV 4.5e-15, du 1.8e-13, value 1.3e-14, dV[1] + dV[0] / 2 exactly 0; the oracle's own Riccati recursion
    against the KKT solve: du 6.3e-14, value 8.5e-15."""
    fig = wr.check_backward(std, N, B, semi)
    print("backward N=%d B=%d semi=%d:" % (N, B, semi), {k: "%.1e" % v for k, v in fig.items()})
    assert fig["oracle_du"] <= 1e-10 and fig["oracle_value"] <= 1e-10      # the two references agree
    for k in ("K", "kff", "dV", "du", "value", "half"):
        assert fig[k] <= 1e-10, (k, fig[k])


@pytest.mark.parametrize("semi", [False, True])
def test_backward_singular_member_and_batch_independence(std, semi):
    """one member with Hinv = 0 under reg = -2 min(R) (Quu = diag(R) + reg is not positive definite): ok = 0, finite outputs; the other members (oracle's Quu
    positive definite at every stage) are bit-identical to a call on each alone and equal the oracle (measured 3.6e-14)"""
    worst = wr.check_backward_branches(std, semi)
    print("backward branches semi=%d: %.1e" % (semi, worst))
    assert worst <= 1e-10


# ---- 2. landing_wb_rollout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nalpha,B", [(1, 1), (2, 8), (5, 7)])
@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("semi", [False, True])
@pytest.mark.parametrize("with_f", [False, True])
def test_rollout_every_slot(std, with_f, semi, closed, nalpha, B):
    """nalpha B = 1, 16, 35 threads: one lane, one full workgroup of WB_TPB, two full workgroups and a ragged one.  Arrow path (structured solve).  Bound 1e-12
    relative to max(1, |.|).  Measured (seed 3, N = 4, worst of the 24 cases): x 2.0e-15, u 2.7e-15, cost 7.3e-15; the 12 cases with foot forces alone x 2.0e-15, u 2.7e-15,
    cost 6.9e-15; the 12 without x 1.9e-15, u 1.4e-15, cost 7.3e-15."""
    fig = wr.check_rollout(std, nalpha, B, 4, with_f, semi, closed)
    print("rollout arrow f=%d semi=%d closed=%d %dx%d:" % (with_f, semi, closed, nalpha, B), {k: "%.1e" % v for k, v in fig.items()})
    assert max(fig.values()) <= 1e-12, fig


@pytest.mark.parametrize("nalpha,B", [(1, 1), (2, 8), (5, 7)])
@pytest.mark.parametrize("semi,closed", [(False, True), (True, True), (False, False)])
def test_rollout_every_slot_generic_tree(perm, semi, closed, nalpha, B):
    """the same on the renumbered quadruped: hand_c_lds follows the parent table, chol_solve18_lds solves.  Measured (worst of the 9 cases): x 1.0e-15, u 1.0e-15,
    cost 3.6e-15"""
    fig = wr.check_rollout(perm, nalpha, B, 4, False, semi, closed, permuted=True)
    print("rollout dense semi=%d closed=%d %dx%d:" % (semi, closed, nalpha, B), {k: "%.1e" % v for k, v in fig.items()})
    assert max(fig.values()) <= 1e-12, fig


@pytest.mark.parametrize("with_f", [False, True])
def test_rollout_skip_mask_is_applied_and_consumed_once(std, with_f):
    wr.check_rollout_skip(std, with_f)


def test_rollout_velocity_update_equals_the_dynamics_kernels(std, perm):
    """the rollout kernel's header: its dynamics are those of hand_c / chol_solve18.  N = 1: qd+ - qd against dt qdd of landing_fb_dynamics_batch to 1e-12.
    On the emulation the dense path (generic tree) IS bit-equal (qd + dt qdd reproduces qd+ exactly); the arrow path is not -- it eliminates the legs first
    (arrow_solve18_lds) and agrees to rounding, 6.4e-16 -- which is what the header now says."""
    e_arrow, bit_arrow = wr.check_rollout_header_claim(std, True)
    e_dense, bit_dense = wr.check_rollout_header_claim(perm, False)
    print("rollout vs dynamics kernels: arrow %.1e bit-equal %s, dense %.1e bit-equal %s" % (e_arrow, bit_arrow, e_dense, bit_dense))
    assert e_arrow <= 1e-12 and e_dense <= 1e-12
    assert bit_dense      # host emulation: no FMA contraction, same order of operations


# ---- 3. landing_wb_select ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nalpha", [1, 4])
@pytest.mark.parametrize("N", [3, 8])
def test_select_against_numpy_restatement(std, N, nalpha):
    """(N + 1) 36 = 144 and 324 elements per member: below and above the 256 threads of the copy loop.  Search mode with and without a step array, keep mode with
    and without members that already hold a step; copies bit-equal, members not picked untouched"""
    wr.check_select(std, N, nalpha)


def test_select_argument_errors(std):
    wr.check_select_argument_errors(std)


# ---- 4. the loop when it backtracks --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,semi", wr.LOOP_CASES)
def test_loop_backtracks_like_the_oracle(name, semi):
    """step-length lists whose first entry overshoots: every member's alphas equal the oracle's, its cost history agrees to 1e-9 relative (measured 2.7e-12),
    the fused two-stage search and the host loop agree bit for bit; "mixed" has an iteration in which one member takes the first entry (stage 1) and the others
    a later one (stage 2).  The record the GPU tests compare with (tests/golden/wb_backtrack.npz) equals the oracle run here."""
    alphas = wr.LOOP_LISTS[name]
    L = _lib()
    fused, host = wr.loop_run(L, "cpu", alphas, semi, True), wr.loop_run(L, "cpu", alphas, semi, False)
    for k in ("alpha", "cost", "x", "u"):
        assert np.array_equal(fused[k], host[k]), k
    al, hist = wr.loop_oracle(alphas, semi)
    print(name, semi, fused["alpha"].tolist(), "cost history vs oracle %.1e" % np.max(np.abs(fused["cost"] - hist) / hist))
    assert np.array_equal(fused["alpha"], al), (fused["alpha"], al)
    assert np.max(np.abs(fused["cost"] - hist) / hist) <= 1e-9
    assert (fused["alpha"] != alphas[0]).any() and (fused["alpha"] != 0.0).all()      # it backtracked, and every member found a step
    if name in ("a", "b"):
        assert (fused["alpha"] != alphas[0]).all()                                    # the issue's lists: never the first entry
    if name == "mixed":
        first = fused["alpha"] == alphas[0]
        assert any(first[it].any() and not first[it].all() for it in range(first.shape[0])), fused["alpha"]
    g_al, g_hist = wr.loop_golden(GOLDEN, name, semi)
    assert np.array_equal(g_al, al) and np.max(np.abs(g_hist - hist) / hist) <= 1e-12


def test_loop_without_iterations_returns_the_initial_rollout():
    """iters = 0 (no backward pass: `expected` is None) == the first row of a longer run's history"""
    import torch
    import test_wb
    L = _lib()
    x0, u0, xref, f = wr.loop_problem()
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    S = lc("wb").WholeBodySQP(L, lc("rbd").Rbd(L), wr.LOOP_N, test_wb.DT, test_wb.Q, test_wb.R, test_wb.QN, device="cpu")
    o0 = S.solve(t(x0), t(u0), t(xref), t(f), iters=0, K_init=test_wb.KPD)
    o1 = S.solve(t(x0), t(u0), t(xref), t(f), iters=1, K_init=test_wb.KPD)
    assert o0["alpha"] is None and o0["expected"] is None and o0["cost"].shape == (1, wr.LOOP_B) and torch.equal(o0["cost"][0], o1["cost"][0])
    assert o1["expected"].shape == (wr.LOOP_B, 2) and bool((o1["expected"][:, 0] < 0).all()) and torch.equal(o1["expected"][:, 1], -0.5 * o1["expected"][:, 0])


# ---- 5. the generic-tree path --------------------------------------------------------------------------------------------------------
def test_generic_tree_dynamics_against_oracle_and_quad_path(perm, std):
    """landing_fb_lin_exact_kernel<false> / rnea_tangent and the generic hand_c on the renumbered quadruped, without foot forces, 3 points (seed 3).  Measured:
    H 2.2e-16, C 1.3e-16, qdd 9.2e-16, Hinv 9.9e-16, exact A 9.8e-10 against the Richardson oracle (whose own accuracy is 1e-8), central-difference A 7.1e-9,
    exact A against the quad path's (rnea_tangent_quad on the standard model, permuted) 2.2e-15."""
    fig = wr.check_generic_tree(perm, std, 3, 3)
    print("generic tree:", {k: "%.1e" % v for k, v in fig.items()})
    for k, bound in wr.GENERIC_BOUNDS.items():
        assert fig[k] <= bound, (k, fig[k])


def test_foot_forces_are_refused_on_a_tree_with_other_leg_numbering(perm, std):
    """hand_c, hand_c_lds and rnea_tangent reach a foot through bodies 0..5 and b_foot-3 .. b_foot-1: on the renumbered tree that is another chain, so
    landing_fb_dynamics_batch and landing_wb_rollout return LANDING_E_ARG when foot forces are given (and the entry points that compose the same chain for
    forward kinematics always); without forces, and on the standard model, nothing changes"""
    q, qd, tau, f = wr.points(np.random.default_rng(0), 2)
    P = wr.PERM
    with pytest.raises(RuntimeError, match=r"\(-1\).*landing_fb_dynamics_batch with foot forces"):
        perm.fb(q[:, P], qd[:, P], tau[:, P], f, want=("C",))
    d = wr.rollout_inputs(1, 4)
    a = ((1.0,), d["x"], d["u"], d["xref"])
    with pytest.raises(RuntimeError, match="landing_wb_rollout with foot forces"):
        perm.rollout(*a, d["f"], None, None, wr.DT, wr.Q, wr.R, wr.QN)
    q6 = np.ascontiguousarray(q[:, :6]); jp = np.ascontiguousarray(q[:, 6:]); out = np.zeros((2, 12)); p = lambda v: v.ctypes.data
    with pytest.raises(RuntimeError, match="landing_kinodyn_rows_batch"):
        perm.rbd.kinodyn_rows(2, p(q6), 0, 0, p(jp), p(out))
    with pytest.raises(RuntimeError, match="landing_leg_ik_batch"):
        perm.rbd.leg_ik(2, p(q6), p(out), p(jp))
    # accepted: the same calls without forces on this tree, and with forces on the standard one
    assert np.isfinite(perm.fb(q[:, P], qd[:, P], tau[:, P], None, want=("C",))["C"]).all()
    assert np.isfinite(perm.rollout(*a, None, None, None, wr.DT, wr.Q, wr.R, wr.QN)[2]).all()
    assert np.isfinite(std.fb(q, qd, tau, f, want=("C",))["C"]).all()
    assert np.isfinite(std.rollout(*a, d["f"], None, None, wr.DT, wr.Q, wr.R, wr.QN)[2]).all()
    std.rbd.kinodyn_rows(2, p(q6), 0, 0, p(jp), p(out))
    assert np.isfinite(out).all() and np.abs(out).max() > 0.0
