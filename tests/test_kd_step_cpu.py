"""CPU tests (host emulation, tests/emu) of the Newton step the kinodynamic refinement solver computes (landing_kd_head_kernel / landing_kd_condense_kernel /
landing_kd_iter_kernel): after a solve stopped at an iteration limit, dx, ds and the defect rows' multipliers in the member's workspace block
(landing_debug_kd_workspace / _layout / _state) must be the solution of the primal-dual Newton system at the point the step was taken from -- solved by
tests/kd_newton_reference.py through the numerics of tests/newton_reference.py (one sparse symmetric system, LU with extended-precision refinement), which shares
nothing with the kernels' table-driven condensation, compact Jacobian blocks, matrix-core stage elimination, terminal cost-to-go and forward sweep.  The SRBM
solver's counterpart is tests/test_solver_step_cpu.py; read its docstring for the construction of the bound.

J of the reference is the complex-step Jacobian of the ORACLE's rows (all columns in one batched call); the product's function-layer Jacobian is held against it
to 1e-11 in every case.  H comes from the product's function layer (landing_kinodyn_nlp_hess; there is no exact oracle Hessian) and is held, every column, against
central differences of the oracle's grad_lagrangian_batch to 1e-6 in one case per test.

Intermediates (kd_step_harness.check_sig_rho / check_gc, every checked step): Sigma / rho of the workspace against the formula in np.longdouble to 4 ulp of the term
sums; every interval's J_I' Sigma J_I and J_I' rho against the np.longdouble restatement over the function layer's Jacobian, per entry min(8 eps, (n + 2) 2^-53) of the
sum of |terms| (n = number of terms of the entry: kd_step_harness.gc_bound), entries no row couples exactly 0 on both sides, and the inequality rows' columns 48..59
(X_k+1) exactly 0.  An entry sums up to 52 products (the diagonal entries of forces and joint angles), not "about a dozen": up to 15 terms the bound is the derived
worst case, beyond that the flat 8 eps holds by measurement -- worst 2.7 eps here, 4.7 eps on the MI355X.

Bound: per quantity, error <= 16 x max(e_aug, e_cond, 1e-15).  Worst measured ratio error / max(e_aug, e_cond, 1e-15) on the emulation (bound: 16):
    first step    N = 2: 4.8    N = 3: 1.9    N = 6: 1.2        (30 cases: five option sets x delta_floor default / 0; every one needs ONE factorisation)
    later steps   N = 6: 0.36                                   (9 pairs, K in {1, 2, 5}, none skipped)
    pending path  N = 6: 0.68                                   (2 pairs: iteration 6 with 7 / 6 factorisations)
Normwise backward error of the kernel's step (printed with -s, not asserted): <= 3.0e-14 first steps, 1.5e-14 later steps, 5.6e-14 pending path.  Product Jacobian
against the complex step: <= 6.7e-16; product Hessian against central differences: <= 3.8e-8.  The device's figures are in tests/test_gpu_kd_step.py.

THE REGULARISATION.  delta sits on the diagonal of every stage block (kd_assemble_stage) and on X_N (kd_terminal): c_1 .. c_{N-1} -- control of one stage, state of
the next -- receive 2 delta, every other free variable delta.  kd_newton_reference.d_reg encodes it; test_plain_delta_identity_is_not_what_the_kernel_solves pins that
delta * I is NOT the system the kernel solves.  delta_floor (3e-4) makes delta > 0 in every iteration, so the convention is observable in every default case.

PENDING PATH.  No FIRST step needs more than one factorisation at these sizes, with delta_floor = 0 either (the multipliers of the defects start at 0).  Running the
emulation over the iteration limits 1 .. 8 with delta_floor = 0 and the slacks pushed 1e-4 (mu_init 1e-2) found members 0 and 3 at N = 6, whose iteration 6 needs
7 / 6 factorisations (delta 0, delta_init, then x delta_inc_first up to 10 / 1): KD_TRIES_PER_ROUND = 2, so the inertia correction returns with `pending` set and
resumes in later launches with the state taken from the workspace.  test_inertia_correction_resumed_in_a_later_launch (PENDING) checks that step and its delta.

What these tests catch, tried on emulation builds of scratch copies of the tree (never committed); tests failing of the 35 of this file:
    one dterm entry of the middle table dropped (KdCPat::dterm[0], destination 300)    3   test_later_steps_are_newton_steps and both pending cases, by the gc check
    one rterm entry of the last-interval table dropped (KdCPat::rterm[1], variable 30)  3   the same three, by the gc check
        (at a first step the dropped products vanish: no first-step case sees these two)
    delta left off X_N in kd_terminal                                                  19   the first steps with delta_floor = 3e-4, the delta * I test, later and pending steps
    KD_ROW2X with two entries swapped                                                  34   every step case (all but the layout test)
    ds of the terminal rows left out in kd_forward                                     34   every step case
None of the five goes unnoticed.
"""
import numpy as np
import pytest

import kd_newton_reference as kr
import kd_step_harness as H
import newton_reference as nr
from conftest import lc
from emu_support import build_emu, emu_landing_lib

HORIZONS = (2, 3, 6)
FLOORS = (None, 0.0)
LATER_K = (1, 2, 5)
LATER_MEMBERS = (0, 1, 2)
# members whose iteration 6 needs 7 / 6 factorisations with the proximal floor off and the slacks pushed 1e-4 (found by running the emulation over iteration limits 1 .. 8):
# (member, K); the inertia correction of iteration K + 1 goes through `pending` and resumes in later launches
PENDING = [(0, 5), (3, 5)]
PENDING_OSET = (1e-4, 1e-2)
WORST = {}


def _first_specs():
    out = []
    for N in HORIZONS:
        for i, oset in enumerate(H.OPTION_SETS):
            for fl in FLOORS:
                out.append(dict(N=N, member=(i + (fl is not None)) % 3, oset=oset, delta_floor=fl, max_iters=[0, 1], tag="N%d-opts%d-floor%s" % (N, i, "0" if fl == 0.0 else "def")))
    return out


FIRST = _first_specs()
LATER = [dict(N=6, member=m, oset=None, delta_floor=None, max_iters=sorted(set(LATER_K) | {k + 1 for k in LATER_K}), tag="later-m%d" % m) for m in LATER_MEMBERS]
LATER += [dict(N=6, member=m, oset=PENDING_OSET, delta_floor=0.0, max_iters=[K, K + 1], tag="pending-m%d" % m) for m, K in PENDING]


@pytest.fixture(scope="module")
def emu_runs(tmp_path_factory):
    """every emulation run of this file, one process per (member, option set), all at once: tag -> (Problem, x0, opts, {max_iter: run})"""
    build_emu()
    specs = FIRST + LATER
    res = H.emu_runs_parallel([{k: v for k, v in s.items() if k != "tag"} for s in specs], tmp_path_factory.mktemp("kd_emu"))
    return {s["tag"]: r for s, r in zip(specs, res)}


def test_layout_is_the_stride_and_entry_points_refuse_without_a_solve():
    L = emu_landing_lib(20); R = lc("rbd").Rbd(L)
    with pytest.raises(Exception):
        R.kinodyn_debug_workspace(1)
    with pytest.raises(Exception):
        R.kinodyn_debug_state(0)
    for N in (2, 20, 64):
        off = R.kinodyn_workspace_layout(N)
        nx, ng = kr.ko.nlp_dims(N)
        assert off["x"] == (0, nx) and off["dx"] == (2 * nx, nx) and off["g"] == (4 * nx, ng)      # kd_carve: x | xt | dx | gx | g | gt | s | ds | zL | zU | y | yn | sig | rho
        names = ["g", None, "s", "ds", "zL", "zU", "y", "yn", "sig", "rho"]
        for i, n in enumerate(names):
            if n:
                assert off[n] == (4 * nx + i * ng, ng)
        assert off["gc"][0] + off["gc"][1] == off["state"] < off["total"] and off["gc"][1] == N * kr.GC
    with pytest.raises(Exception):
        R.kinodyn_workspace_layout(65)
    L.close()


@pytest.mark.parametrize("spec", FIRST, ids=[s["tag"] for s in FIRST])
def test_first_step_is_the_newton_step(emu_runs, spec):
    """max_iter = 1, portfolio off, no feasibility phase: the state the step is taken from is fully determined by the inputs (kd_newton_reference.initial_state), and
    run 0 (max_iter = 0) shows that the kernels start there"""
    pr, x0, opts, runs = emu_runs[spec["tag"]]
    N = pr.N
    v, rec = H.member_view(runs[1], 0)
    assert runs[1]["res"]["iters"][0] == 1 and runs[1]["res"]["status"][0] == 1 and rec["it"] == 1, (runs[1]["res"]["status"], rec)
    nfact = int(rec["nfact"])
    assert rec["delta"] == nr.delta_schedule(opts, nfact, opts.delta_floor), (rec["delta"], nfact)
    assert opts.delta_floor == (3e-4 if spec["delta_floor"] is None else 0.0)
    xs, step = kr.start_point(pr, x0), rec["alpha"] * v["dx"]
    assert (np.abs(runs[1]["res"]["x"][0] - (xs + step)) <= 4 * kr.EPS * (np.abs(xs) + np.abs(step))).all(), "x_1 = x_0 + alpha dx"
    first_of_N = spec["tag"].endswith("opts0-floordef")
    skip, worst, bwd = H.check_pair(pr, x0, runs, 0, 0, "first " + spec["tag"], jac="oracle", opts=opts, hess_check=first_of_N)
    assert skip is None, skip
    key = "first N%d" % N
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print("first step %s: %d factorisations, delta %.3g, worst ratio %.3g (N %d so far %.3g), gc %.2f eps" % (spec["tag"], nfact, rec["delta"], worst, N, WORST[key], H.WORST_GC[0]))


def test_plain_delta_identity_is_not_what_the_kernel_solves(emu_runs):
    """with D_reg = delta * I the kernel's step misses the bound: the feet c_1 .. c_{N-1} carry 2 delta.  If this test fails, the kernel's regularisation has changed:
    update kd_newton_reference.d_reg, landing_nlp.h and DESIGN.md with it."""
    pr, x0, opts, runs = emu_runs["N6-opts0-floordef"]
    v, rec = H.member_view(runs[1], 0)
    assert rec["delta"] == opts.delta_floor == 3e-4
    st = kr.initial_state(pr, x0, opts); st["y"] = runs[0]["res"]["lam_g"][0]
    J = kr.jacobian_complex_step(pr, st["x"]); Hm = kr.hessian_from_blocks(pr.N, runs[0]["Hb"][0])
    H.check_step(pr, st, v, rec, J, Hm, label="2 delta on the feet")
    with pytest.raises(AssertionError):
        H.check_step(pr, st, v, rec, J, Hm, dreg=kr.d_reg_plain(pr.N, rec["delta"]), label="delta * I")
    ref = kr.solve_step(pr, st, rec["mu"], kr.d_reg_plain(pr.N, rec["delta"]), J, Hm)
    err = nr.errors(ref, v["dx"], v["ds"], v["yn"])
    assert err["dx"] > 1e3 * nr.bounds_of(ref)["dx"]
    # the kernel's stationarity residual in the delta * I system is +delta dx on the feet and rounding elsewhere
    a = ref["a"]; n = a["n"]; free = ref["free"]
    y = np.array(v["yn"][24:]); I = a["ineq"]; y[I] = a["sig"][I] * v["ds"][24:][I] + a["bar"][I]
    z = np.concatenate([v["dx"][free], y])
    r = nr._res_ld(ref["K"].tocoo(), z, ref["b"]).astype(float)[:n]
    feet = np.searchsorted(free, kr.foot_twice(pr.N)); other = np.setdiff1d(np.arange(n), feet)
    scale = 64 * kr.EPS * float((abs(ref["K"]) @ np.abs(z))[:n].max())
    assert np.abs(rec["delta"] * v["dx"][free][feet]).max() > 1e3 * scale
    assert np.abs(r[feet] - rec["delta"] * v["dx"][free][feet]).max() <= scale and np.abs(r[other]).max() <= scale


def test_later_steps_are_newton_steps(emu_runs):
    """K in {1, 2, 5}, three members at N = 6: run K gives the state (x, lam_g, s / zL / zU of the workspace), run K + 1 from the same inputs the step (dx, ds, yn, gc, the
    record's mu and delta); the Hessian is then taken at non-zero defect multipliers.  Skipped: a member that stopped earlier, a restart between the two runs
    (nreset / last_reset_it differ); at most one pair in five.  On the emulation none is skipped."""
    checked, skipped, worst = 0, [], 0.0
    for m in LATER_MEMBERS:
        pr, x0, opts, runs = emu_runs["later-m%d" % m]
        for K in LATER_K:
            skip, w, _ = H.check_pair(pr, x0, runs, K, 0, "later N 6 K %d member %d" % (K, m), jac="oracle", hess_check=(m == 0 and K == 5))
            if skip:
                skipped.append(skip); print("skipped:", skip)
            else:
                checked += 1; worst = max(worst, w)
        assert max(abs(r["res"]["lam_g"][0][48:60]).max() for r in runs.values()) > 1e-3      # the defect multipliers are non-zero
    WORST["later"] = worst
    print("later steps N 6: %d pairs checked, skipped %s, worst ratio %.3g, gc %.2f eps (most terms %d)" % (checked, skipped, worst, H.WORST_GC[0], H.WORST_GC[1]))
    assert checked + len(skipped) == len(LATER_MEMBERS) * len(LATER_K) and len(skipped) * 5 <= checked + len(skipped), skipped


@pytest.mark.parametrize("case", PENDING, ids=["m%d" % c[0] for c in PENDING])
def test_inertia_correction_resumed_in_a_later_launch(emu_runs, case):
    """an iteration that needs >= 3 factorisations (delta_floor = 0: the schedule starts at 0): after KD_TRIES_PER_ROUND = 2 failures the iteration kernel returns with
    `pending` set and a later launch resumes the inertia correction from the state in the workspace.  The step it finally takes is the Newton step at the record's delta,
    and that delta is the schedule's value at the factorisation count (no regularisation before: the schedule starts afresh)."""
    m, K = case
    pr, x0, opts, runs = emu_runs["pending-m%d" % m]
    _, reck = H.member_view(runs[K], 0); _, recn = H.member_view(runs[K + 1], 0)
    nf = int(recn["nfact"] - reck["nfact"])
    assert nf >= 3 and reck["delta_last"] == 0.0 and reck["nfact"] == K, (nf, reck)
    assert recn["delta"] == nr.delta_schedule(opts, nf, 0.0) and recn["delta"] > 0.0 and recn["pending"] == 0, (recn["delta"], nf)
    skip, worst, _ = H.check_pair(pr, x0, runs, K, 0, "pending member %d K %d" % (m, K), jac="oracle")
    assert skip is None, skip
    WORST["pending"] = max(WORST.get("pending", 0.0), worst)
    print("pending path member %d: %d factorisations in iteration %d, delta %.3g, worst ratio %.3g (so far %.3g)" % (m, nf, K + 1, recn["delta"], worst, WORST["pending"]))
