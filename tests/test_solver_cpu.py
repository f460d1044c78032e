"""CPU tests of the solver layer (no GPU):
  * the oracle's CPU port converges to KKT <= 1e-6 (its own lo_kkt) on seeded drop states and reproduces the
    reference's golden known answer (f* <= 2e-5 for test_scripts/1.5msDrop30Pitch.mat);
  * the HIP solver kernel, compiled for the host through tests/emu (same sources, fibers instead of lanes),
    follows the CPU port iterate for iterate -- table-driven condensation, Riccati sweep with the in-register
    elimination, filter line search are all exercised without a GPU.
"""
import os

import numpy as np
import pytest

import certificate_reference as cr
from conftest import GOLDEN, lc
from emu_support import build_emu, emu_landing_lib


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu()


def test_cpu_port_converges_and_certifies(oracle_mod):
    N = 20
    O = oracle_mod.Oracle(N)
    P, X0, _, _ = lc("problem").make_batch(3, N, 0.6, seed=1)
    r = oracle_mod.cpu_solve_batch(O, P, X0, threads=3, max_iter=400)
    assert (r["status"] == 0).all()
    for b in range(3):
        assert O.kkt(r["x"][b], P[b], r["lam_g"][b]).max() <= 1e-6 * 1.0001
        assert np.allclose(r["kkt"][b], O.kkt(r["x"][b], P[b], r["lam_g"][b]))


def test_cpu_port_golden_known_answer(oracle_mod):
    O = oracle_mod.Oracle(20)
    d = np.load(os.path.join(GOLDEN, "n20_golden_1p5ms30pitch.npz"))
    p = d["p"]; o = O.param_offsets()
    _, x0, _, _ = lc("problem").make_member(20, 0.6, p[o["q_init"]:o["q_init"] + 6], p[o["qd_init"]:o["qd_init"] + 6])
    r = oracle_mod.cpu_solve_batch(O, p[None], x0[None], threads=1, max_iter=600)
    assert r["status"][0] == 0 and O.f(r["x"][0], p) <= 2e-5     # reference optimum f* in [0, 1.64e-5]


def test_cpu_port_reference_default_problem(oracle_mod):
    """BASELINE configs[0]: the drop the generator script solves itself (generate_landingCtrller_IPOPT.m:173-224);
    its terminal reference is reachable, so the optimum is f* = 0."""
    O = oracle_mod.Oracle(20)
    p, x0 = lc("problem").reference_default_problem()
    r = oracle_mod.cpu_solve_batch(O, p[None], x0[None], threads=1, max_iter=600)
    assert r["status"][0] == 0 and O.f(r["x"][0], p) <= 1e-8
    assert O.kkt(r["x"][0], p, r["lam_g"][0]).max() <= 1e-6 * 1.0001


@pytest.mark.parametrize("clip_k,theta_floor", [(4, 30.0), (1, 0.0)])      # the defaults; IPOPT's classic step rule and filter tests
def test_emulated_kernel_follows_cpu_port(emu_lib, oracle_mod, clip_k, theta_floor):
    N, K = 20, 6
    O = oracle_mod.Oracle(N)
    P, X0, _, _ = lc("problem").make_batch(1, N, 0.6, seed=1)
    L = lc("capi").LandingLib(N, lib_path=emu_lib)
    o = L.default_opts(); o.max_iter = K; o.clip_k = clip_k; o.theta_floor = theta_floor; o.feas_phase = 0      # (K iterations, then stop: no feasibility phase)
    classic = dict(dual_step_cap=0.0, fresh_restart=0, slack_corr=0.0, watchdog=0, barrier_smax=0.0) if clip_k == 1 else {}
    for k_, v_ in classic.items():
        setattr(o, k_, v_)
    assert (L.default_opts().clip_k, L.default_opts().theta_floor) == (4, 30.0)
    g = L.solve_host(P, X0, o)
    c = oracle_mod.cpu_solve_batch(O, P, X0, threads=1, max_iter=K, clip_k=clip_k, theta_floor=theta_floor, feas_phase=0, **classic)
    assert g["status"][0] == 1 and c["status"][0] == 1 and g["iters"][0] == c["iters"][0] == K
    assert np.max(np.abs(g["x"][0] - c["x"][0])) < 1e-7 * max(1.0, np.max(np.abs(c["x"][0])))
    assert np.max(np.abs(g["lam_g"][0] - c["lam_g"][0])) < 1e-6 * max(1.0, np.max(np.abs(c["lam_g"][0])))
    # the kernel's own KKT report is the reference-consistent residual
    assert np.allclose(g["kkt"][0], O.kkt(g["x"][0], P[0], g["lam_g"][0]), rtol=1e-6, atol=1e-12)


def test_max_iter_zero_stops_at_once_in_kernel_and_port(emu_lib, oracle_mod):
    """with max_iter <= 0 the feasibility phase used to set its iteration limit BEHIND the counter (lim = it + max_iter, it + 1
    next) and the kernel's `it == lim` test could never fire: an unbounded loop on the GPU.  Both solvers now stop at once -- status
    MAX_ITER, no iteration, the initial guess returned -- with the default options (feasibility phase on)."""
    N = 20
    O = oracle_mod.Oracle(N)
    P, X0, _, _ = lc("problem").make_batch(2, N, 0.6, seed=3)
    L = lc("capi").LandingLib(N, lib_path=emu_lib)
    for mi in (0, -5):
        o = L.default_opts(); o.max_iter = mi
        assert o.feas_phase == 1
        g = L.solve_host(P, X0, o)
        c = oracle_mod.cpu_solve_batch(O, P, X0, threads=1, max_iter=mi)
        assert (g["status"] == 1).all() and (c["status"] == 1).all()
        assert (g["iters"] == 0).all() and (c["iters"] == 0).all()
        assert np.array_equal(g["x"][:, 12:], X0[:, 12:])
    o = L.default_opts(); o.max_iter = 1      # one iteration, then the phase gets one iteration as well and the solve ends
    g = L.solve_host(P, X0, o)
    c = oracle_mod.cpu_solve_batch(O, P, X0, threads=1, max_iter=1)
    assert (g["status"] == 1).all() and np.array_equal(g["iters"], c["iters"]) and (g["iters"] <= 3).all()


def test_emulated_kernel_long_horizon(emu_lib, oracle_mod):
    """N = 80 (> 64 stages: the lane = stage phases run in two chunks, sigma_0..80 of the forward sweep fill the LDS array; limit 96): the
    emulated kernel follows the CPU port"""
    N, K = 80, 3
    O = oracle_mod.Oracle(N)
    P, X0, _, _ = lc("problem").make_batch(1, N, 0.6, seed=4)
    L = lc("capi").LandingLib(N, lib_path=emu_lib)
    o = L.default_opts(); o.max_iter = K; o.feas_phase = 0
    g = L.solve_host(P, X0, o)
    c = oracle_mod.cpu_solve_batch(O, P, X0, threads=1, max_iter=K, feas_phase=0)
    assert g["iters"][0] == c["iters"][0] == K
    assert np.max(np.abs(g["x"][0] - c["x"][0])) < 1e-9 and np.max(np.abs(g["lam_g"][0] - c["lam_g"][0])) < 1e-7
    L100 = lc("capi").LandingLib(100, lib_path=emu_lib)
    P, X0, _, _ = lc("problem").make_batch(1, 100, 0.6, seed=4)
    with pytest.raises(RuntimeError, match="N <= 96"):
        L100.solve_host(P, X0)


RUN_COST = dict(QX=[0, 0, 10, 1, 1, 0, .1, .1, .1, .1, .1, .1], Qc=[1.0, 1.0, 0.5], Qf=[1e-4, 1e-4, 1e-3], f_ref=[0, 0, 20.0])


def test_running_cost_oracle_gradient_and_port(oracle_mod):
    """running cost of the reference's N=41 script (generate_quadruped_SRBM_CCC.m:81-89): the oracle's gradient against central
    differences, and the CPU port converging to a KKT point of that objective"""
    N = 20
    O = oracle_mod.Oracle(N, run_cost=RUN_COST); O0 = oracle_mod.Oracle(N)
    P, X0, _, _ = lc("problem").make_batch(2, N, 0.6, seed=1)
    x = X0[0] + 0.01 * np.random.default_rng(0).normal(size=O.nx)
    g = np.asarray(O.grad_f(x, P[0])[-1] if isinstance(O.grad_f(x, P[0]), tuple) else O.grad_f(x, P[0])).ravel()
    assert O.f(x, P[0]) > O0.f(x, P[0])
    for i in np.random.default_rng(1).choice(O.nx, 60, replace=False):
        e = np.zeros(O.nx); e[i] = 1e-6
        assert abs((O.f(x + e, P[0]) - O.f(x - e, P[0])) / 2e-6 - g[i]) < 1e-6 * max(1.0, abs(g[i]))
    r = oracle_mod.cpu_solve_batch(O, P, X0, threads=2, max_iter=400)
    assert (r["status"] == 0).all()
    for b in range(2):
        assert O.kkt(r["x"][b], P[b], r["lam_g"][b]).max() <= 1e-6 * 1.0001


def test_emulated_kernel_follows_cpu_port_with_running_cost(emu_lib, oracle_mod):
    N, K = 20, 6
    O = oracle_mod.Oracle(N, run_cost=RUN_COST)
    P, X0, _, _ = lc("problem").make_batch(1, N, 0.6, seed=1)
    L = lc("capi").LandingLib(N, lib_path=emu_lib, run_cost=RUN_COST)
    o = L.default_opts(); o.max_iter = K; o.feas_phase = 0
    g = L.solve_host(P, X0, o)
    c = oracle_mod.cpu_solve_batch(O, P, X0, threads=1, max_iter=K, feas_phase=0)
    assert g["iters"][0] == c["iters"][0] == K
    assert np.max(np.abs(g["x"][0] - c["x"][0])) < 1e-7 * max(1.0, np.max(np.abs(c["x"][0])))
    assert np.allclose(g["kkt"][0], O.kkt(g["x"][0], P[0], g["lam_g"][0]), rtol=1e-6, atol=1e-12)
    assert abs(g["f"][0] - O.f(g["x"][0], P[0])) < 1e-10 * max(1.0, abs(g["f"][0]))


def test_fp32_factor_option_is_retired_and_ignored(emu_lib, capfd):
    """landing_solver_opts::factor_fp32 (the single-precision stage elimination of rounds 2-4) was retired in round 5 -- slower than the
    fp64 factor on every measurement (include/landing_nlp.h): the field stays in the struct, callers that still set it get the fp64
    factor (the very same iterates) and one warning on stderr"""
    N = 20
    P, X0, _, _ = lc("problem").make_batch(1, N, 0.6, seed=1)
    L = lc("capi").LandingLib(N, lib_path=emu_lib)
    o = L.default_opts(); o.max_iter = 2; o.feas_phase = 0; o.factor_fp32 = 1
    a = L.solve_host(P, X0, o)
    assert "factor_fp32 is retired" in capfd.readouterr().err
    o.factor_fp32 = 0
    b = L.solve_host(P, X0, o)
    assert a["iters"][0] == b["iters"][0] == 2 and np.array_equal(a["x"], b["x"])


def test_clip_rule_changes_the_path_and_shortens_it(oracle_mod):
    """landing_solver_opts::clip_k (CPU port = the kernel's algorithm, test above): with the 4th most blocking slack setting the step
    length a seeded set of N = 40 drop states needs fewer iterations than with IPOPT's classic rule, and both end at KKT points"""
    N = 40
    O = oracle_mod.Oracle(N)
    P, X0, _, _ = lc("problem").make_batch(8, N, 0.6, seed=20211)
    a = oracle_mod.cpu_solve_batch(O, P, X0, threads=8, max_iter=300)
    b = oracle_mod.cpu_solve_batch(O, P, X0, threads=8, max_iter=300, clip_k=1, theta_floor=0.0, dual_step_cap=0.0, fresh_restart=0, slack_corr=0.0, watchdog=0, barrier_smax=0.0)
    assert (a["status"] == 0).all() and (b["status"] == 0).all()
    assert a["iters"].sum() < b["iters"].sum(), (a["iters"], b["iters"])
    for r in (a, b):
        for m in range(8):
            assert O.kkt(r["x"][m], P[m], r["lam_g"][m]).max() <= 1e-6 * 1.0001


def test_feasibility_phase_rescues_or_certifies(oracle_mod):
    """landing_solver_opts::feas_phase (the restoration phase of the reference's IPOPT, as a solve of the elastic problem with the same
    machinery): on a hard small-horizon batch the emulated kernel follows the CPU port -- members that ended NUMERICAL / MAX_ITER are either
    rescued (KKT <= 1e-6 under the oracle's functions) or certified locally infeasible (status 3: equality rows met, positive violation that
    equals the kernel's report); members that converge without the phase are the same bits with it."""
    N, B = 10, 6
    O = oracle_mod.Oracle(N)
    L = emu_landing_lib(N)
    P, X0, _, _ = lc("problem").make_batch(B, N, 0.6, seed=3)
    keep = [1, 3, 5]; P, X0, B = P[keep], X0[keep], 3      # (one member of each kind: certified, rescued, converged anyway -- the emulation is slow)
    o = L.default_opts(); o.max_iter = 150
    o.mu_init = 0.1; o.bound_push = 0.5; o.theta_mu = 1.5; o.kappa_eps = 80.0      # the three members were picked under these values (the defaults are automatic since round 4)
    assert o.feas_phase == 1 and o.feas_rho == 1000.0
    r1 = L.solve_host(P, X0, o)
    o.feas_phase = 0
    r0 = L.solve_host(P, X0, o)
    c1 = oracle_mod.cpu_solve_batch(O, P, X0, threads=4, max_iter=150, feas_phase=1, mu_init=0.1, bound_push=0.5, theta_mu=1.5, kappa_eps=80.0)
    assert (r0["status"] != 0).sum() == 2                                    # two of the three fail without the phase
    assert np.array_equal(r1["status"], c1["status"]), (r1["status"], c1["status"])
    assert (r1["status"] == 0).sum() > (r0["status"] == 0).sum() and (r1["status"] == 3).sum() >= 1
    same = r0["status"] == 0
    assert np.array_equal(r0["x"][same], r1["x"][same]) and np.array_equal(r0["iters"][same], r1["iters"][same])
    for b in range(B):
        if r1["status"][b] == 0:
            assert O.kkt(r1["x"][b], P[b], r1["lam_g"][b]).max() <= 1e-6 * 1.0001
        if r1["status"][b] == 3:
            g = O.g(r1["x"][b], P[b]); lb, ub = O.bounds(P[b]); eq = lb == ub
            viol = np.maximum(np.maximum(lb - g, g - ub), 0.0)
            assert np.abs(g[eq] - lb[eq]).max() <= 1e-6 and abs(viol.max() - r1["kkt"][b, 0]) <= 1e-12 and viol.sum() > 1e-4
            assert np.abs(r1["x"][b] - c1["x"][b]).max() <= 1e-6             # the CPU port ends at the same elastic KKT point
            for r_ in (r1, c1):      # ... which IS one, with the multipliers each returns (tests/certificate_reference.py: E, S, B, V, C, P)
                res = cr.srbm_certificate(O, r_["x"][b], P[b], r_["lam_g"][b], o.feas_rho, o.tol, feas_cert=o.feas_cert, kkt0=r_["kkt"][b, 0], kkt0_atol=1e-12)
                assert cr.failed(res) == [], (b, res)
    L.close()


def test_feas_jam_and_stat_cut_the_production_tail(emu_lib, oracle_mod):
    """landing_solver_opts::feas_jam / feas_stat (round 5) on the reference's production problem (N = 20, non-uniform grid, data-generation
    law): the feasibility phase starts when the line search jams instead of at the iteration limit, and ends when the violation is
    stationary.  CPU port on 256 drop states: the slowest member needs far fewer iterations, nobody who converged without the phase changes
    a bit, the members left undecided do not become more; and the emulated kernel follows the port through both rules on a member that
    ends with a certificate of local infeasibility after 130 instead of ~500 iterations."""
    N = 20
    Pm = lc("problem")
    O = oracle_mod.Oracle(N)
    P, X0, _, _ = Pm.make_batch(1024, N, 0.6, seed=100000, consts=Pm.production_constants("datagen"), dt_grid="reference", law="datagen")
    P, X0 = P[:256], X0[:256]
    new = oracle_mod.cpu_solve_batch(O, P, X0, threads=8, max_iter=300)
    old = oracle_mod.cpu_solve_batch(O, P, X0, threads=8, max_iter=300, feas_jam=0, feas_stat=0)
    print("iterations max %d -> %d, mean %.1f -> %.1f; converged %d -> %d, certified %d -> %d, undecided %d -> %d" % (
        old["iters"].max(), new["iters"].max(), old["iters"].mean(), new["iters"].mean(), (old["status"] == 0).sum(), (new["status"] == 0).sum(),
        (old["status"] == 3).sum(), (new["status"] == 3).sum(), np.isin(old["status"], (1, 2)).sum(), np.isin(new["status"], (1, 2)).sum()))
    assert new["iters"].max() <= 0.8 * old["iters"].max() and new["iters"].sum() < old["iters"].sum()
    assert np.isin(new["status"], (1, 2)).sum() <= np.isin(old["status"], (1, 2)).sum()
    assert (new["status"] == 0).sum() >= (old["status"] == 0).sum() - 3
    quick = (old["status"] == 0) & (old["iters"] < 100) & (new["iters"] == old["iters"])      # never near either rule
    assert quick.sum() >= 230 and np.array_equal(new["x"][quick], old["x"][quick])
    for b in np.nonzero(new["status"] == 3)[0]:
        g = O.g(new["x"][b], P[b]); lb, ub = O.bounds(P[b]); eq = lb == ub
        viol = np.maximum(np.maximum(lb - g, g - ub), 0.0)
        assert np.abs(g[eq] - lb[eq]).max() <= 1e-6 * 1.0001 and abs(viol.max() - new["kkt"][b, 0]) <= 1e-9 and viol.sum() > 1e-4      # (round 6: status 3 = elastic KKT point, nothing else)
        res = cr.srbm_certificate(O, new["x"][b], P[b], new["lam_g"][b], 1000.0, 1e-6, kkt0=new["kkt"][b, 0])      # ... with multipliers that prove it
        assert cr.failed(res) == [], (b, res)
    m = 131      # certified early by the new rules (416 iterations without them); member 40 is another one, but behind its first early return (round 6) it passes through a
    assert new["status"][m] == 3 and new["iters"][m] < 200 and old["iters"][m] > 300      # region with pr ~ 50 where the kernel's and the port's roundings part ways
    L = lc("capi").LandingLib(N, lib_path=emu_lib)
    o = L.default_opts(); o.max_iter = 300
    assert (o.feas_jam, o.feas_stat) == (8, 25)
    g = L.solve_host(P[m:m + 1], X0[m:m + 1], o)
    assert g["status"][0] == 3 and g["iters"][0] == new["iters"][m]
    assert np.abs(g["x"][0] - new["x"][m]).max() <= 1e-5 and abs(g["kkt"][0, 0] - new["kkt"][m, 0]) <= 1e-7
    assert (o.feas_rho, o.tol, o.feas_cert) == (1000.0, 1e-6, 1e-4)      # (what the port's certificates were held to above) ... and the kernel's own multipliers prove the same
    assert cr.failed(cr.srbm_certificate(O, g["x"][0], P[m], g["lam_g"][0], o.feas_rho, o.tol, feas_cert=o.feas_cert, kkt0=g["kkt"][0, 0])) == []
    L.close()


def test_round6_phase_rules_kernel_follows_port(emu_lib, oracle_mod):
    """Round 6 (landing_nlp.h: feas_back / feas_max / feas_delta_dec / feas_ret_push / feas_resume / feas_polish): the feasibility phase
    the way IPOPT runs its restoration phase -- an early entry returns as soon as the violation has come down, up to three entries, the point handed
    back is taken over warm, status 3 ONLY at a KKT point of the elastic problem (equality rows <= 1e-6), a stationary violation is polished once and
    otherwise ends as LANDING_STALLED (4).  Three members of the reference's production problem (data-generation law), one per path, through the
    emulated kernel and the CPU port: same status, same iteration count, same point.
      * (100000, 145): jam at ~60, phase, early return, converges after 93 iterations (rounds 3-5 rules: 386);
      * (100000, 592): ends at an elastic KKT point with positive violation: certificate, equality rows <= 1e-6 under the oracle;
      * (7, 94): the third phase stalls, the polishing step does not make it a KKT point, the resumed iteration jams again: status 4."""
    N = 20
    Pm = lc("problem")
    O = oracle_mod.Oracle(N)
    L = lc("capi").LandingLib(N, lib_path=emu_lib)
    o = L.default_opts(); o.max_iter = 300
    assert (o.feas_back, o.feas_max, o.feas_delta_dec, o.feas_ret_push, o.feas_ret_mu, o.feas_resume, o.feas_polish) == (0.2, 3, 0.1, 0.01, 0.01, 1, 1e-8)
    for seed, m, status in ((100000, 145, 0), (7, 94, 4)):      # ((100000, 592): status 3 after 146 iterations, checked when the rules were ported; the certificate path is also test_feas_jam_and_stat's member 131)
        P, X0, _, _ = Pm.make_batch(1024, N, 0.6, seed=seed, consts=Pm.production_constants("datagen"), dt_grid="reference", law="datagen")
        c = oracle_mod.cpu_solve_batch(O, P[m:m + 1], X0[m:m + 1], threads=1, max_iter=300)
        g = L.solve_host(P[m:m + 1], X0[m:m + 1], o)
        assert c["status"][0] == status and g["status"][0] == status and g["iters"][0] == c["iters"][0], (seed, m, c["status"], g["status"], c["iters"], g["iters"])
        assert np.abs(g["x"][0] - c["x"][0]).max() <= 1e-3 and abs(g["kkt"][0, 0] - c["kkt"][0, 0]) <= 1e-7
        gg = O.g(g["x"][0], P[m]); lb, ub = O.bounds(P[m]); eq = lb == ub
        viol = np.maximum(np.maximum(lb - gg, gg - ub), 0.0)
        if status == 0:
            assert O.kkt(g["x"][0], P[m], g["lam_g"][0]).max() <= 1e-6 * 1.0001
            old = oracle_mod.cpu_solve_batch(O, P[m:m + 1], X0[m:m + 1], threads=1, max_iter=300, feas_max=1, feas_back=0.0, feas_delta_dec=0.0, feas_ret_push=0.0, feas_resume=0, feas_polish=0.0, feas_jam=0, feas_stat=0)
            assert old["iters"][0] >= 3 * c["iters"][0]
        if status == 3:
            assert np.abs(gg[eq] - lb[eq]).max() <= 1e-6 and abs(viol.max() - g["kkt"][0, 0]) <= 1e-9 and viol.sum() > 1e-4
        res = [cr.srbm_certificate(O, r_["x"][0], P[m], r_["lam_g"][0], o.feas_rho, o.tol, feas_cert=o.feas_cert, kkt0=r_["kkt"][0, 0]) for r_ in (g, c)] if status in (3, 4) else None
        if status == 3:
            assert cr.failed(res[0]) == [] and cr.failed(res[1]) == [], res
        if status == 4:
            assert abs(viol.max() - g["kkt"][0, 0]) <= 1e-9
            assert cr.failed(res[0]) != [] and cr.failed(res[1]) != []      # a stalled member is no certificate: the check tells the two apart
    L.close()


def test_stag_relief_shortens_the_known_slow_member(oracle_mod):
    """landing_solver_opts::stag_relief (round 4): member 304 of the bench batch (seed 20211) reaches pr ~ 1e-5 after 36 iterations and then takes 45 FULL
    Newton steps to 1e-6 -- the proximal term delta_floor against a curvature of ~1e-5.  With the rule (default 3) the floor shrinks once three such steps have
    not halved the error; both runs end at KKT points under the oracle's functions.  (CPU port = the kernel's algorithm, test_kernel_matches_cpu_port.)"""
    N = 40
    O = oracle_mod.Oracle(N)
    P, X0, _, _ = lc("problem").make_batch(1024, N, 0.6, seed=20211)
    P, X0 = P[304:305], X0[304:305]
    sched = dict(kappa_eps=80.0, theta_mu=1.5)      # the barrier schedule the member was found with (the automatic one moved on: 120 / 1.8)
    a = oracle_mod.cpu_solve_batch(O, P, X0, threads=1, max_iter=300, stag_relief=0, jam_clip=0, **sched)
    b = oracle_mod.cpu_solve_batch(O, P, X0, threads=1, max_iter=300, **sched)
    assert a["status"][0] == 0 and b["status"][0] == 0
    assert a["iters"][0] >= 80 and b["iters"][0] <= 60, (a["iters"], b["iters"])      # measured: 88 -> 52
    for r in (a, b):
        assert O.kkt(r["x"][0], P[0], r["lam_g"][0]).max() <= 1e-6 * 1.0001
