"""Certificates of local infeasibility (status LANDING_INFEASIBLE) held to the KKT conditions of the elastic problem (no GPU).

include/landing_nlp.h defines the status as a KKT point of the elastic problem with positive violation; callers drop such drop states for good.
tests/certificate_reference.py restates those conditions on plain arrays -- equality rows (E), J' lam = 0 (S), multiplier bounds and signs (B), the full
price on every violated row (V), complementarity inside the bounds (C), positive violation = the reported one (P) -- with bounds derived from the stop
test, not from either solver.  Here: the checker against a problem solved by hand, the CPU port's certificates on the reference's production problem,
a control that must FAIL (the stationary-violation exit that rounds 3-5 reported under this status), and the HIP solver kernel itself, compiled for
the host through tests/emu, with the multipliers it returns."""
import numpy as np
import pytest

import certificate_reference as cr
from conftest import lc
from emu_support import build_emu

RHO, TOL = 1000.0, 1e-6
N = 20


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu()


def _production(seed):
    Pm = lc("problem")
    P, X0, _, _ = Pm.make_batch(1024, N, 0.6, seed=seed, consts=Pm.production_constants("datagen"), dt_grid="reference", law="datagen")
    return P, X0


@pytest.fixture(scope="module")
def port(oracle_mod):
    """the CPU port on the first 256 members of seeds 100000 and 3 (+ member 592 of the first), once for the module: seed -> (P, X0, result)"""
    O = oracle_mod.Oracle(N)
    out = {}
    for seed in (100000, 3):
        P, X0 = _production(seed)
        sel = np.arange(256) if seed == 3 else np.concatenate([np.arange(256), [592]])
        out[seed] = (P[sel], X0[sel], oracle_mod.cpu_solve_batch(O, P[sel], X0[sel], threads=16, max_iter=300))
    return O, out


def _n10(oracle_mod):
    P, X0, _, _ = lc("problem").make_batch(6, 10, 0.6, seed=3)
    return oracle_mod.Oracle(10), P[1:2], X0[1:2], dict(mu_init=0.1, bound_push=0.5, theta_mu=1.5, kappa_eps=80.0)      # (the options of test_feasibility_phase_rescues_or_certifies)


def _compl(O, x, p, lam):
    """max |lam_r| x distance to the bound lam_r pushes against, on the NLP's bounds (what kkt[2] is defined as, landing_nlp.h d_kkt)"""
    g = O.g(np.ascontiguousarray(x), np.ascontiguousarray(p)); lb, ub = O.bounds(np.ascontiguousarray(p))
    with np.errstate(invalid="ignore"):
        dist = np.where(lam > 0.0, ub - g, g - lb)
    use = (lb != ub) & (lam != 0.0) & np.isfinite(dist)
    return np.abs(lam[use] * dist[use]).max()


def _kkt12(O, r, b, p, rho, tol):
    """kkt[1] and kkt[2] of a certificate as landing_nlp.h (d_kkt) defines them: the elastic problem's dual infeasibility, <= tol; max |lam| dist of the returned
    (x, lam_g) on the NLP's bounds, which is rho x kkt[0] to first order: at most (rho + tol) v on a violated row and tol (1 + rho) + tol / width inside (B, C of
    certificate_reference), at least (rho - tol - tol / (v - tol) - tol / width) v on the most violated row (V; v / (v - tol) <= 100 / 99 above its floor)."""
    k = r["kkt"][b]
    assert k[1] <= tol * 1.0001, k
    assert abs(k[2] - _compl(O, r["x"][b], p, r["lam_g"][b])) <= 1e-9 * k[2], k
    lb, ub = O.bounds(np.ascontiguousarray(p))
    two = (lb != ub) & np.isfinite(lb) & np.isfinite(ub)
    width = (ub - lb)[two].min()
    t = tol * 1.0001
    assert k[0] > 100 * tol
    assert k[2] <= max((rho + t) * k[0], t * (1 + rho) + t / width) and k[2] >= rho * k[0] - t * (k[0] + 100.0 / 99.0 + k[0] / width), (k, width)


# ---- a: the checker against a problem solved by hand ------------------------------------------------------------------------------------

def _hand(x, lam):
    """x in R^2, five linear rows:   r0  x1 - x2 = 0          r1  2 x2 >= 2          r2  -3 <= x1 <= 0 (two-sided)
                                     r3  -5 <= x2 <= 5         r4  x1 + x2 <= 3.
    r1 and r2 contradict each other through r0.  On the line x1 = x2 = t the violation is 2 (1 - t)+ + t+: smallest at t = 1 (value 1, r2 violated by 1,
    r1 met with equality, r3 inside by 4, r4 inside by 1).  Multipliers there: r2 carries the price, lam2 = +rho; column x1: lam0 + lam2 + lam4 = 0;
    column x2: -lam0 + 2 lam1 + lam3 + lam4 = 0; lam3 = lam4 = 0 (inside)  =>  lam0 = -rho, lam1 = -rho / 2 (one-sided lower row: <= 0, |.| <= rho)."""
    J = np.array([[1.0, -1.0], [0.0, 2.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    lb = np.array([0.0, 2.0, -3.0, -5.0, -np.inf]); ub = np.array([0.0, np.inf, 0.0, 5.0, 3.0])
    g = J @ np.asarray(x, float)
    v = np.maximum(np.maximum(lb - g, g - ub), 0.0)[1:]
    return cr.certificate_residuals(g, lb, ub, np.asarray(lam, float), RHO, TOL, J=J, kkt0=v.max())


def test_checker_on_a_problem_solved_by_hand():
    x, lam = np.array([1.0, 1.0]), np.array([-RHO, -RHO / 2, RHO, 0.0, 0.0])
    res = _hand(x, lam)
    assert cr.failed(res) == [], res
    assert res["P"]["value"] == 1.0 and res["P"]["v1"] == 1.0 and res["V"]["rows"] == 1 and res["V"]["row"] == 2 and res["E"]["rows"] == 1
    # the same point from the sparse form and from J' lam, |J|' |lam| handed over
    import scipy.sparse as sp
    J = np.array([[1.0, -1.0], [0.0, 2.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    lb = np.array([0.0, 2.0, -3.0, -5.0, -np.inf]); ub = np.array([0.0, np.inf, 0.0, 5.0, 3.0])
    for kw in (dict(J=sp.csc_matrix(J)), dict(Jt_lam=J.T @ lam, absJt_abslam=np.abs(J).T @ np.abs(lam))):
        r2 = cr.certificate_residuals(J @ x, lb, ub, lam, RHO, TOL, kkt0=1.0, **kw)
        assert cr.failed(r2) == [] and r2["S"]["bound"] == res["S"]["bound"]
    # a multiplier inside the allowances passes: rho - |lam| of the violated row may be tol + tol / (v - tol) + tol / (ub - lb)
    d = 0.9 * (TOL + TOL / (1.0 - TOL) + TOL / 3.0)
    assert cr.failed(_hand(x, [-(RHO - d), -(RHO - d) / 2, RHO - d, 0.0, 0.0])) == []
    # 1. the violated row's multiplier at 0.9 rho (the others follow, so that J' lam stays 0): only V
    assert cr.failed(_hand(x, [-0.9 * RHO, -0.45 * RHO, 0.9 * RHO, 0.0, 0.0])) == ["V"]
    # 2. a multiplier of the wrong sign on a one-sided row (r4 has no lower bound: lam4 >= 0; the others follow): B, and nothing about stationarity
    bad = _hand(x, [-RHO + 1e-3, -RHO / 2 + 1e-3, RHO, 0.0, -1e-3])
    assert "B" in cr.failed(bad) and "S" not in cr.failed(bad) and bad["B"]["sign"] == 1e-3 and bad["B"]["row"] == 4
    assert "B" in cr.failed(_hand(x, [-RHO, RHO / 2, RHO, 0.0, 0.0]))      # ... r1 has no upper bound: lam1 <= 0
    assert "B" in cr.failed(_hand(x, [-1.1 * RHO, -0.55 * RHO, 1.1 * RHO, 0.0, 0.0]))      # ... and more than the price
    # 3. a multiplier on the slack row r4, at distance 1 from its bound (the others follow): only C
    dl = 1e-3
    assert cr.failed(_hand(x, [-RHO - dl, -RHO / 2 - dl, RHO, 0.0, dl])) == ["C"]
    assert cr.failed(_hand(x, [-RHO - TOL / 2, -RHO / 2 - TOL / 2, RHO, 0.0, TOL / 2])) == []      # (|lam| dist = tol / 2 is within the bound)
    # 4. a point moved to where the violation still has a descent direction (t = 0.5: r1 and r2 both violated, d violation / dt = -1), with the multipliers the
    #    violated rows must carry and the best lam0 there is: no multiplier vector makes it stationary
    xm = np.array([0.5, 0.5])
    fails = cr.failed(_hand(xm, [-1.5 * RHO, -RHO, RHO, 0.0, 0.0]))      # (lam0 = least squares of lam0 + rho = 0, -lam0 - 2 rho = 0)
    assert fails == ["S"], fails
    # 5. the equality row off by 10 tol: only E
    assert cr.failed(_hand([1.0 + 10 * TOL, 1.0], lam)) == ["E"]
    # P: a violation below feas_cert is no certificate; a reported kkt[0] that is not the violation is not one either
    J0 = _hand(x, lam)
    assert J0["P"]["ok"]
    g = J @ x
    assert cr.failed(cr.certificate_residuals(g, lb, ub, lam, RHO, TOL, J=J, kkt0=1.0 + 1e-6)) == ["P"]
    assert cr.failed(cr.certificate_residuals(g, lb, ub, lam, RHO, TOL, J=J, kkt0=1.0, feas_cert=2.0)) == ["P"]


# ---- b, c: the CPU port ---------------------------------------------------------------------------------------------------------------------

def test_cpu_port_certificates_are_elastic_kkt_points(port, oracle_mod):
    """Every status-3 member of the CPU port -- production problem N = 20, data-generation law, first 256 members of seeds 100000 and 3, member (100000, 592),
    and N = 10 member 1 of make_batch(6, 10, 0.6, seed=3) -- passes all six residuals; at least 4 certificates per seed (the port gives 40, 120, 131, 154, 252 and 7, 63, 76, 95, 187, 189; and 592).
    Worst values over the 13 certificates (bounds in brackets): E 3.2e-7 (1e-6), S 2.1e-8 (1e-6), |lam| <= 1000 (1000 + 1e-6), V rho - |lam| 3.3e-4 (its
    bound on that row: 3.3e-3), C 1.0e-7 (1e-6): V and C sit at the last barrier parameter tol / 10, a factor 10 inside their bounds, as they should.
    kkt[1] of a certificate is the elastic problem's dual infeasibility (<= tol) and kkt[2] = max |lam| dist on the NLP's bounds (landing_nlp.h d_kkt)."""
    O, runs = port
    W = cr.Worst()
    for seed, (P, X0, r) in runs.items():
        cert = np.nonzero(r["status"] == 3)[0]
        assert (cert < 256).sum() >= 4, (seed, cert)
        print("seed %d: certificates %s" % (seed, [int(b) if b < 256 else 592 for b in cert]))
        for b in cert:
            res = cr.srbm_certificate(O, r["x"][b], P[b], r["lam_g"][b], RHO, TOL, kkt0=r["kkt"][b, 0])
            assert cr.failed(res) == [], (seed, b, res)
            _kkt12(O, r, b, P[b], RHO, TOL)
            W.add(res)
    O10, P, X0, opts = _n10(oracle_mod)
    r = oracle_mod.cpu_solve_batch(O10, P, X0, threads=1, max_iter=150, feas_phase=1, **opts)
    assert r["status"][0] == 3
    res = cr.srbm_certificate(O10, r["x"][0], P[0], r["lam_g"][0], RHO, TOL, kkt0=r["kkt"][0, 0])
    assert cr.failed(res) == [], res
    W.add(res)
    print("CPU port:", W)


def test_stationary_violation_exit_fails_the_check(port, oracle_mod):
    """The control.  With feas_polish = 0, feas_resume = 0 member (100000, 120) ends where rounds 3-5 reported status 3: a violation that has been stationary for
    feas_stat iterations.  It is status 4 now and it is NOT an elastic KKT point: E 9.3e-5 and S 9.6e-6 against 1e-6 (V and C miss too).  Member (7, 94), status 4
    under the defaults, fails as well.  The check tells a stationary-violation exit from a certificate."""
    O, runs = port
    P, X0, _ = runs[100000]
    r = oracle_mod.cpu_solve_batch(O, P[120:121], X0[120:121], threads=1, max_iter=300, feas_polish=0.0, feas_resume=0)
    assert r["status"][0] == 4
    res = cr.srbm_certificate(O, r["x"][0], P[120], r["lam_g"][0], RHO, TOL, kkt0=r["kkt"][0, 0])
    print("control (100000, 120): E %.1e S %.1e, fails %s" % (res["E"]["value"], res["S"]["value"], cr.failed(res)))
    assert "E" in cr.failed(res) and "S" in cr.failed(res)
    assert res["E"]["value"] > 10 * TOL and res["S"]["value"] > 5 * TOL      # (not a near miss: 93 tol and 9.6 tol)
    P7, X7 = _production(7)
    r = oracle_mod.cpu_solve_batch(O, P7[94:95], X7[94:95], threads=1, max_iter=300)
    assert r["status"][0] == 4
    res = cr.srbm_certificate(O, r["x"][0], P7[94], r["lam_g"][0], RHO, TOL, kkt0=r["kkt"][0, 0])
    assert cr.failed(res) != [], res


# ---- d: the HIP solver kernel through tests/emu ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["100000/131", "100000/592", "n10/1"])
def test_emulated_kernel_certificates_are_elastic_kkt_points(emu_lib, port, oracle_mod, case):
    """landing_ipm_kernel, compiled for the host, on three members that end with a certificate: status 3, and the point with the multipliers THE KERNEL returns
    (lam_g = zU - zL of the elastic rows, the fixed initial rows from stationarity) passes all six residuals, rho / tol / feas_cert read from the options struct.
    kkt[1] is the elastic problem's dual infeasibility (<= tol, and not below |J' lam| over the free variables, which is part of it), kkt[2] = max |lam| dist
    on the NLP's bounds; the CPU port reports the same three numbers (landing_nlp.h d_kkt).
    Emulation, worst of the three: E 8.2e-9  S 6.5e-10  rho - |lam| 3.3e-4 (bound on that row 3.3e-3)  C 1.0e-7.
    MUTATIONS of the sources, each run through this test in a scratch copy (never committed): (A) e.dw scaled by 0.5 in el_step -> all three members end NUMERICAL, the test
    fails on the status; (B) the c_rn term dropped from ipm_errors -> the SAME BITS come back (z + w - rho is a linear row: one full Newton step zeroes it, and the last
    steps are full), an equivalent mutant on these members that no test of the output can see; (C) the objective leaking into the phase's derivatives (lam_f 0.05
    instead of 0) -> all three end MAX_ITER, fails on the status; (D) the fixed rows' multipliers written as -0.999 grad instead of -grad -> status 3 as before and the
    test fails on S (1.0 against 1e-6), on nothing else."""
    if case == "n10/1":
        O, P, X0, opts = _n10(oracle_mod)
        max_iter, Nc = 150, 10
    else:
        seed, m = (int(s) for s in case.split("/"))
        O, runs = port
        b = m if m < 256 else 256
        P, X0, opts, max_iter, Nc = runs[seed][0][b:b + 1], runs[seed][1][b:b + 1], {}, 300, N
    L = lc("capi").LandingLib(Nc, lib_path=emu_lib)
    o = L.default_opts(); o.max_iter = max_iter
    for k_, v_ in opts.items():
        setattr(o, k_, v_)
    assert (o.feas_phase, o.feas_rho, o.tol, o.feas_cert) == (1, RHO, TOL, 1e-4)
    g = L.solve_host(P, X0, o)
    L.close()
    c = oracle_mod.cpu_solve_batch(O, P, X0, threads=1, max_iter=max_iter, **opts)
    assert g["status"][0] == 3 and c["status"][0] == 3, (g["status"], c["status"])
    res = cr.srbm_certificate(O, g["x"][0], P[0], g["lam_g"][0], o.feas_rho, o.tol, feas_cert=o.feas_cert, kkt0=g["kkt"][0, 0])
    print("emulated kernel %s: %s" % (case, {n: "%.2e (%.2e)" % (res[n]["value"], res[n]["bound"]) for n in cr.NAMES}))
    assert cr.failed(res) == [], res
    import scipy.sparse as sp
    _, jv = O.jac_g(np.ascontiguousarray(g["x"][0]), np.ascontiguousarray(P[0])); ci, r = O.pattern_jac()
    free = np.abs(sp.csc_matrix((jv, r, ci), shape=(O.ng, O.nx)).T @ g["lam_g"][0])[12:].max()
    for s in (g, c):
        _kkt12(O, s, 0, P[0], o.feas_rho, o.tol)
    assert g["kkt"][0, 1] >= free - res["S"]["rounding"]


# ---- e: the kinodynamic refinement kernels through tests/emu --------------------------------------------------------------------------------

def test_emulated_kinodynamic_kernels_phase_certificate_is_an_elastic_kkt_point(emu_lib):
    """landing_kd_head / condense / iter / finish kernels, compiled for the host, on a 2-interval member that no solver can land: flat attitude, v_z = -5 m/s, dt = 50 ms.
    The interior-point iteration runs into its limit (30), the feasibility phase ends at a KKT point of the elastic problem: status 3 after 59 iterations (iters > 0: a
    PHASE certificate, not the presolve one).  With the multipliers the finish kernel writes -- y of the elastic rows, the 24 fixed rows from stationarity -- the point
    passes the six residuals under the oracle's rows and complex-step Jacobian, and kkt[1] is the elastic problem's dual infeasibility (landing_nlp.h d_kkt).
    Emulation: E 1.6e-11  S 3.9e-12  rho - |lam| 1.3e-6 (bound on that row 1.4e-5)  C 1.0e-7.  (N <= 4 candidates with a steep attitude end in the
    presolve certificate or at the iteration limit; the portfolio's clone path needs four members x 200 iterations and stays on the GPU: tests/test_gpu_kd_solver.py.)"""
    kd, P = lc("kinodyn"), lc("problem")
    mass, Ib, Ibi = lc("constants").robot_constants(); Ib, Ibi = np.asarray(Ib), np.asarray(Ibi)
    Ns, dtv = 2, np.full(2, 0.05)
    Ls = lc("capi").LandingLib(Ns, lib_path=emu_lib); Rs = lc("rbd").Rbd(Ls)
    q = np.array([0, 0, 0.0, 0.0, 0.0, 0.0]); qd = np.array([0.0, 0.0, 0.0, 0.0, 0.0, -5.0])
    q[2] = 0.35 + abs(min((kd.rot_xyz(q[3:6]) @ np.array([sx * 0.19, sy * 0.1, 0.0]))[2] for sx in (1, -1) for sy in (1, -1))) + abs(dtv[0] * qd[5])
    _, x0s, _, _ = P.make_member(Ns, 0.3, q, qd, P.production_constants("main"), dtv)
    lb, ub, cost, x0 = kd.member_problem(Ns, q, qd, x0s)
    o = Rs.kinodyn_default_opts(); o.max_iter = 30; o.kd_clone_after = 0
    assert (o.feas_phase, o.feas_rho, o.tol, o.feas_cert) == (1, RHO, TOL, 1e-4)
    s = Rs.kinodyn_solve_host(Ns, lb, ub, cost, x0, dtv, mass, Ib, Ibi, 0.75, o)
    Ls.close()
    assert s["status"][0] == 3 and s["iters"][0] > o.max_iter, (s["status"], s["iters"], s["kkt"])
    res = cr.kd_certificate(s["x"][0], s["lam_g"][0], lb, ub, Ns, dtv, mass, Ib, Ibi, 0.75, o.feas_rho, o.tol, feas_cert=o.feas_cert, kkt0=s["kkt"][0, 0])
    print("emulated kinodynamic kernels: %d iterations, %s" % (s["iters"][0], {n: "%.2e (%.2e)" % (res[n]["value"], res[n]["bound"]) for n in cr.NAMES}))
    assert cr.failed(res) == [], res
    assert s["kkt"][0, 1] <= o.tol * 1.0001 and s["kkt"][0, 0] > 100 * o.tol
