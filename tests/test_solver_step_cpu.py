"""CPU tests (host emulation, tests/emu) of the Newton step landing_ipm_kernel computes: after a launch, dx, ds and the equality multipliers
in the member's workspace block must be the solution of the primal-dual Newton system at the point the step was taken from -- solved by
tests/newton_reference.py (one sparse symmetric system, LU with extended-precision refinement), which shares nothing with the kernel's
table-driven condensation, blocked Riccati sweep, forward sweep and row products.  The CPU port of oracle/ is no such check: it is the same
recursion by the same hand (and it regularises the same way, see below).

Bound (newton_reference.py): per quantity, error <= 16 x max(e_aug, e_cond, 1e-15), where e_aug / e_cond are the forward errors of unrefined
fp64 sparse LU solves of the augmented / the condensed system of the very same step -- what an fp64 method of either structure achieves.
Worst measured ratio error / max(e_aug, e_cond, 1e-15) on the emulation (bound: 16):
    first step        2.0   (bound_push = mu_init = 1e-6 and bound_push = 1e-8: equality multipliers; dx / ds stay below 0.2)
    regularised step  0.45
    later steps       0.32
The device's figures are in tests/test_gpu_solver_step.py and DESIGN.md ("Newton-step check").  The normwise backward error of the kernel's
step in the augmented system is printed for every case (run with -s) and not asserted: <= 1e-17 here.

What these tests catch (tried on scratch copies): delta applied once to c_k in the reference -- every case with delta > 0 fails (20 of 32);
one condensation term of one stage scaled by 1 + 1e-9 -- 11 of 31 fail; RIC_MV read one entry off in the forward sweep -- all 31 fail.

THE REGULARISATION.  delta_w is added to the diagonal of every stage block, so the feet c_1 .. c_{N-1} -- control of stage k, state of
stage k + 1 -- receive 2 delta (include/landing_nlp.h delta_init).  newton_reference.d_reg encodes it;
test_plain_delta_identity_is_not_what_the_kernel_solves pins that delta * I is NOT the system the kernel solves, so the convention cannot
drift silently.  The CPU port adds delta over the same stage blocks (landing_solver_cpu.c riccati_backward), i.e. it shares the convention --
which is why the emulated-kernel-follows-port tests never saw it.

Inertia (test_regularised_step_and_inertia): in both cases examined the augmented matrix has the right inertia (n_free, n_rows, 0) at the
accepted delta and the wrong one at the previous value of the schedule and at delta = 0, so that is asserted.
"""
import numpy as np
import pytest

import newton_reference as nr
import solver_step_harness as H
from conftest import lc
from emu_support import build_emu

RC_CCC = dict(QX=[0.3, 0.2, 10, 1, 1, 0.4, .1, .2, .1, .3, .1, .2], Qc=[1.0, 0.8, 0.5], Qf=[1e-4, 2e-4, 1e-3], f_ref=[0.5, -0.25, 20.0])
WORST = {}


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu()


def problem(form, N, B, seed, **kw):
    """(oracle, library keyword arguments, P, X0) of a form: "plain" (terminal cost), "rc" (running cost, constants of the context),
    "ccc" (running cost with the N=41 script's own parameter vector)"""
    from oracle.oracle import Oracle
    Pm = lc("problem")
    P, X0, _, _ = Pm.make_batch(B, N, 0.6, seed=seed, **kw)
    if form == "plain":
        return Oracle(N), {}, P, X0
    if form == "rc":
        return Oracle(N, run_cost=H.RUN_COST), dict(run_cost=H.RUN_COST), P, X0
    rng = np.random.default_rng(seed)
    Pc = np.zeros((B, Pm.n_p_ccc(N)))
    for b in range(B):
        Uref = X0[b][12 * (N + 1):].reshape(24, N, order="F").copy()
        Uref[12:] = np.tile(RC_CCC["f_ref"], 4)[:, None] + 0.3 * rng.normal(size=(12, N))
        Pc[b] = Pm.ccc_from_ipopt_params(N, P[b], Uref, RC_CCC["QX"], RC_CCC["Qc"], RC_CCC["Qf"])
    return Oracle(N, run_cost=RC_CCC, ccc_params=True), dict(run_cost=RC_CCC, ccc_params=True), Pc, X0


@pytest.mark.parametrize("N", [3, 20, 64, 96])
@pytest.mark.parametrize("form", ["plain", "rc"])
def test_workspace_offsets_total_is_the_stride(emu_lib, N, form):
    capi = lc("capi")
    L = capi.LandingLib(N, lib_path=emu_lib, **(dict(run_cost=H.RUN_COST) if form == "rc" else {}))
    off = L.workspace_offsets()
    assert off["total"] == L.workspace_stride() == capi.workspace_offsets(N)["total"]
    assert off["rec"] == (off["total"] - 8, 8) and off["y2"][0] + off["y2"][1] == off["rec"][0]
    pos = 0
    for name, part in off.items():      # contiguous, in carve()'s order
        if name != "total":
            assert part[0] == pos; pos += part[1]
    L.close()


def grid(law):
    return dict(dt_grid="reference", law=law, consts=lc("problem").production_constants(law))


# (id, form, N, members, seed, make_batch keywords, option set, delta_floor (None = default))
FIRST = [("N%d" % N, "plain", N, 1 if N > 40 else 2, 10 + N, {}, (1e-2, 0.1), None) for N in (3, 20, 40, 64, 65, 80, 96)]
FIRST += [("opts%d-floor%s" % (i, "0" if fl == 0.0 else "def"), "plain", 20, 2, 5, {}, oset, fl) for i, oset in enumerate(H.OPTION_SETS) for fl in (None, 0.0) if not (i == 0 and fl is None)]
FIRST += [("N96-push1e-8-floor0", "plain", 96, 1, 7, {}, (1e-8, 1e-4), 0.0), ("N65-warm", "plain", 65, 1, 8, {}, "warm", None), ("N40-auto", "plain", 40, 2, 9, {}, None, None),
          ("grid-main", "plain", 20, 2, 100000, grid("main"), (1e-2, 0.1), None), ("grid-datagen", "plain", 20, 2, 100000, grid("datagen"), (1e-4, 1e-2), None),
          ("grid-datagen-warm", "plain", 20, 2, 7, grid("datagen"), "warm", 0.0),
          ("rc-N20", "rc", 20, 2, 1, {}, (1e-2, 0.1), None), ("rc-N40-push1e-6", "rc", 40, 1, 2, {}, (1e-6, 1e-6), None), ("rc-N80-auto", "rc", 80, 1, 3, {}, None, None),
          ("ccc-N20", "ccc", 20, 2, 4, {}, (1e-4, 1e-2), None), ("ccc-N40-warm", "ccc", 40, 1, 5, {}, "warm", None)]


@pytest.mark.parametrize("case", FIRST, ids=[c[0] for c in FIRST])
def test_first_step_is_the_newton_step(emu_lib, case):
    """max_iter = 1, no feasibility phase: the state the step is taken from is fully determined by the inputs (newton_reference.initial_state)"""
    name, form, N, B, seed, kw, oset, floor = case
    O, libkw, P, X0 = problem(form, N, B, seed, **kw)
    L = lc("capi").LandingLib(N, lib_path=emu_lib, **libkw)
    worst, nfact, _ = H.first_step_group(L, O, P, X0, H.step_opts(L, oset, 1, floor), name, plain_form=(form == "plain"))
    WORST["first"] = max(WORST.get("first", 0.0), worst)
    print("first step %s: worst ratio %.3g (so far %.3g), factorisations %s" % (name, worst, WORST["first"], nfact.tolist()))
    L.close()


def test_plain_delta_identity_is_not_what_the_kernel_solves(emu_lib):
    """The finding: with D_reg = delta * I the kernel's step is off by ~1e-6 relative, and its stationarity residual in that system is
    exactly -delta * dx on the feet c_1 .. c_{N-1} and rounding elsewhere -- they carry 2 delta.  If this test fails, the kernel's
    regularisation has changed: update d_reg, landing_nlp.h and DESIGN.md with it."""
    N = 20
    O, _, P, X0 = problem("plain", N, 1, 1)
    L = lc("capi").LandingLib(N, lib_path=emu_lib)
    opts = H.step_opts(L, (1e-2, 0.1))
    run = H.kernel_run(L, P, X0, opts)
    v, rec = H.member_view(run, 0)
    assert rec["delta"] == opts.delta_floor == 3e-4
    st = nr.initial_state(O, P[0], X0[0], opts)
    H.check_step(O, P[0], st, v, rec, label="2 delta on the feet")
    with pytest.raises(AssertionError):
        H.check_step(O, P[0], st, v, rec, dreg=nr.d_reg_plain(N, rec["delta"]), label="delta * I")
    ref = nr.solve_step(O, P[0], st, rec["mu"], nr.d_reg_plain(N, rec["delta"]))
    err = nr.errors(ref, v["dx"], v["ds"], v["yn"])
    assert err["dx"] > 1e3 * nr.bounds_of(ref)["dx"] and 1e-7 < err["dx"] < 1e-5
    a = ref["a"]; n = a["n"]
    y = np.array(v["yn"][12:]); I = a["ineq"]; y[I] = a["sig"][I] * v["ds"][12:][I] + a["bar"][I]
    z = np.concatenate([v["dx"][12:], y])
    r = nr._res_ld(ref["K"].tocoo(), z, ref["b"]).astype(float)
    feet = nr.foot_twice(N) - 12
    other = np.setdiff1d(np.arange(n), feet)
    scale = 64 * np.finfo(float).eps * float((abs(ref["K"]) @ np.abs(z))[:n].max()) / 1e-12      # rounding of one row of K z, as a multiple of the 1e-12 below
    assert np.abs(rec["delta"] * v["dx"][12:][feet]).max() > 1e-8
    assert np.abs(r[feet] - rec["delta"] * v["dx"][12:][feet]).max() <= 1e-12 * scale      # residual b - K z = +delta dx: the kernel's matrix has delta more there
    assert np.abs(r[other]).max() <= 1e-12 * scale and np.abs(r[n:] * np.where(I, a["sig"], 1.0)).max() <= 1e-11 * scale
    L.close()


# members whose FIRST factorisation of iteration K + 1 fails when the proximal floor is off (found with the CPU port's trace): (N, seed, B, member, K)
REGULARISED = [(20, 1, 6, 5, 9), (20, 3, 6, 1, 9)]


@pytest.mark.parametrize("case", REGULARISED, ids=["seed%d-m%d" % (c[1], c[3]) for c in REGULARISED])
def test_regularised_step_and_inertia(emu_lib, tmp_path, case):
    """a step whose first factorisation fails (delta_floor = 0: the schedule starts at 0): the reference with the record's delta, and the
    inertia of the augmented matrix by a dense LDL' -- right at the accepted delta, wrong at the previous value of the schedule and at 0"""
    N, seed, B, m, K = case
    from oracle.oracle import Oracle
    O = Oracle(N)
    P, X0, runs = H.emu_runs_parallel(N, seed, B, (K, K + 1), tmp_path, members=[m], delta_floor=0.0)
    nfact = int(runs[K + 1]["prof"][0, 8] - runs[K]["prof"][0, 8])
    assert nfact >= 2, nfact
    worst, n, skipped = H.later_step_pairs(runs, O, P, "regularised seed %d member %d" % (seed, m))
    assert n == 1 and not skipped
    WORST["reg"] = max(WORST.get("reg", 0.0), worst)
    vk, _ = H.member_view(runs[K], 0); _, recn = H.member_view(runs[K + 1], 0)
    L = lc("capi").LandingLib(N, lib_path=emu_lib); opts = H.step_opts(L, None, delta_floor=0.0); L.close()
    sched = [nr.delta_schedule(opts, i, 0.0) for i in range(1, nfact + 1)]      # (the earlier iterations needed none: the schedule starts afresh)
    assert recn["delta"] == sched[-1] and recn["delta"] > 0.0, (recn["delta"], sched)
    st = dict(x=runs[K]["res"]["x"][0], y=runs[K]["res"]["lam_g"][0], s=vk["s"], zL=vk["zL"], zU=vk["zU"])
    want = (O.nx - 12, O.ng - 12, 0)
    got = {d: nr.inertia_dense(nr.solve_step(O, P[0], st, recn["mu"], nr.d_reg(N, d), refine=0)) for d in (sched[-1], sched[-2], 0.0)}
    print("regularised step seed %d member %d: %d factorisations, delta %s, inertia %s (right: %s), worst ratio %.3g" % (seed, m, nfact, sched, got, want, worst))
    assert got[sched[-1]] == want
    assert got[sched[-2]] != want and got[0.0] != want


LATER_SEEDS = {20: 1, 40: 20211}


@pytest.mark.parametrize("N", [20, 40])
def test_later_steps_are_newton_steps(emu_lib, tmp_path, N):
    """K in {1, 2, 5, 12, 25}, three members: run K gives the state (x, lam_g, live s / zL / zU by the record's flag), run K + 1 from the same
    inputs the step (dx, ds, yn, the record's mu and delta); the Hessian is then taken at non-zero dynamics multipliers.  An iteration in
    which no step is computed (restart) is skipped; at most one pair in five may be.  On the emulation none is skipped."""
    from oracle.oracle import Oracle
    O = Oracle(N)
    Ks = sorted(set(H.LATER_K) | {k + 1 for k in H.LATER_K})
    P, X0, runs = H.emu_runs_parallel(N, LATER_SEEDS[N], 3, Ks, tmp_path)
    worst, n, skipped = H.later_step_pairs(runs, O, P, "later N %d" % N)      # (the pairs (K, K + 1) present in Ks are exactly those of LATER_K)
    WORST["later"] = max(WORST.get("later", 0.0), worst)
    print("later steps N %d: %d pairs checked, skipped %s, worst ratio %.3g" % (N, n, skipped, worst))
    assert n + len(skipped) == 3 * len(H.LATER_K) and len(skipped) * 5 <= n + len(skipped), skipped
    assert max(abs(r["res"]["lam_g"][:, 36:48]).max() for r in runs.values()) > 1e-3      # dynamics multipliers are non-zero
