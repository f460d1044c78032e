"""SURVEY 8(f) row N1 -- the kinodynamic oracle and the kernels pinned to the reference's own MULTIPLIERS.

optimizations/landing/main_scripts/prevSoln.mat holds X_star, U_star, jpos_star and lam_g_star [2844] of a KNITRO solve of the production problem
(landing_optimization.m:386,395; 2844 = ng of 20 intervals).  Posed the way this project poses that problem (production grid, mu 0.75, QN, terminal
reference z = 0.25, kd.bounds at its defaults), (x*, lam*) must be a KKT point of oracle/kinodyn_oracle.py to the 1e-6 the project's own solutions are
certified to.  That is a statement about the row ORDER, the row SIGNS, the Jacobian and the multiplier sign convention together: a consistent error shared by the
oracle and the kernels, which no kernel-against-oracle test can see, breaks it.  What the vector can tell apart is measured here: the whole sign, the grid, mu, the
terminal reference, a shift by one row, and -- group by group -- 19 of the 27 row groups; the other 8 carry multipliers <= ~1e-5 in this solve and stay
pinned by feasibility only.  The kernels (CasADi-external face, Hessian blocks) are then checked AT that point through tests/emu, where the contact and
complementarity rows are active and lam* has the structure of a real solve.  Device counterparts: tests/test_gpu_kd_multipliers.py."""
import numpy as np

import kd_reference_kkt as K
from conftest import lc
from emu_support import emu_landing_lib

N, KKT_TOL, MU = K.N, K.KKT_TOL, K.MU


def _emu_lib():
    return emu_landing_lib(N)


def test_reference_multipliers_are_a_kkt_point_under_the_oracle():
    """primal, dual and complementarity <= 1e-6 each; the dual residual by two derivative mechanisms (Richardson differences, complex step) that agree to 1e-9.
    Measured: primal 4.35e-7 (an Euler defect), dual 3.03e-7 (both), complementarity 2.8e-7; 20 rows whose multiplier pushes an infinite bound, max 5.5e-8."""
    from oracle import kinodyn_oracle as ko
    mass, Ib, Ibi = K.consts()
    pr = K.Problem("m")
    g = pr.g()
    viol = np.maximum(np.maximum(pr.lb - g, g - pr.ub), 0.0)
    f, gf = pr.grad_f()
    du_rich = np.abs(gf + ko.nlp_jacobian(pr.x, N, pr.dt, mass, Ib, Ibi, MU).T @ pr.lam).max()
    du_cs = pr.stationarity(pr.lam)[0]
    lam, eq = pr.lam, pr.lb == pr.ub
    pushed = np.where(lam > 0, pr.ub, pr.lb)                                   # lam > 0 pushes against ubg, lam < 0 against lbg (oracle/kinodyn_oracle.py::kkt)
    act = ~eq & (lam != 0.0)
    fin = act & np.isfinite(pushed)
    co = (np.abs(lam[fin]) * np.maximum(np.where(lam[fin] > 0, pr.ub[fin] - g[fin], g[fin] - pr.lb[fin]), 0.0)).max()
    free = act & ~np.isfinite(pushed)
    print("reference (x*, lam*): f %.2e; primal %.3e (row %d); dual %.4e (Richardson) %.4e (complex step); complementarity %.3e; %d rows push an infinite bound, max |lam| %.2e;"
          " |lam| > 1e-6 on %d rows, max %.4f" % (f, viol.max(), int(np.argmax(viol)), du_rich, du_cs, co, free.sum(), np.abs(lam[free]).max(), (np.abs(lam) > 1e-6).sum(), np.abs(lam).max()))
    assert viol.max() <= KKT_TOL and du_rich <= KKT_TOL and du_cs <= KKT_TOL and co <= KKT_TOL
    assert abs(du_rich - du_cs) <= 1e-9
    assert np.abs(lam[free]).max() <= 1e-7
    assert 0.0 <= f <= 1e-10
    # the same three numbers from the certificate every solver test uses
    k = ko.kkt_batch(pr.x[None], np.where(free, 0.0, lam)[None], N, pr.dt, mass, Ib, Ibi, MU, pr.lb, pr.ub, gf[None])[0]
    assert k.max() <= KKT_TOL and abs(k[0] - viol.max()) <= 1e-15 and abs(k[2] - co) <= 1e-15, k


def test_reference_multipliers_discriminate_sign_grid_friction_and_cost():
    """the KKT residual max(primal, dual) answers to what it is supposed to pin: >= 100 x the unperturbed one (4.35e-7 primal, 3.03e-7 dual) with -lam*, on the
    uniform grid dt = 0.03, with mu 0.5 / 1.0, with the terminal reference z = 0.2 and with lam* shifted by one row in either direction.  Measured (primal | dual):
    -lam* 4.4e-7 | 1.83e-4 (x 420; x 604 dual against dual); dt = 0.03 1.08 | 1.5e-5 (x 2.5e6: the Euler defects -- the dual residual alone moves x 51 only);
    mu 0.5 and 1.0 7.8e-5 dual (x 179; x 257 dual against dual); z 0.2 10 dual (x 2e7); rolled +1 / -1 2.85 / 0.149 dual (x 6.5e6 / x 3.4e5)"""
    pr = K.Problem("m")
    def residual(lam, dt=None, mu=MU, z_ref=None):
        g = pr.g(dt=dt, mu=mu)
        return float(np.maximum(np.maximum(pr.lb - g, g - pr.ub), 0.0).max()), float(pr.stationarity(lam, dt=dt, mu=mu, z_ref=z_ref)[0])
    base = residual(pr.lam)
    cases = {"-lam*": residual(-pr.lam), "dt = 0.03": residual(pr.lam, dt=np.full(N, 0.03)), "mu 0.5": residual(pr.lam, mu=0.5), "mu 1.0": residual(pr.lam, mu=1.0),
             "terminal z 0.2": residual(pr.lam, z_ref=0.2), "lam* rolled +1": residual(np.roll(pr.lam, 1)), "lam* rolled -1": residual(np.roll(pr.lam, -1))}
    print("unperturbed: primal %.3e dual %.4e" % base)
    for name, v in cases.items():
        print("  %-16s primal %.3e dual %.3e  (x %.3g)" % (name, v[0], v[1], max(v) / max(base)))
    assert max(base) <= KKT_TOL
    for name, v in cases.items():
        assert max(v) >= 100.0 * max(base), (name, v, base)
    for name in ("-lam*", "mu 0.5", "mu 1.0", "terminal z 0.2", "lam* rolled +1", "lam* rolled -1"):      # these are statements about the DUAL residual
        assert cases[name][1] >= 100.0 * max(base), (name, cases[name], base)


def test_reference_multipliers_pin_19_of_the_27_row_groups():
    """negating the multipliers of ONE row group lifts the residual to >= 1e-5 for exactly the groups of K.PINNED; the groups of K.UNPINNED carry multipliers too
    small to tell (if a change makes one of them distinguishable this test says so: move it over)"""
    pr = K.Problem("m")
    groups = K.row_groups()
    names = K.PINNED + K.UNPINNED
    lams = np.repeat(pr.lam[None], len(names), axis=0)
    for i, name in enumerate(names):
        lams[i, groups == name] *= -1.0
    res = pr.stationarity(lams)
    for name, r in zip(names, res):
        print("  %-14s rows %4d  max |lam*| %.3e  residual with the group negated %.3e" % (name, (groups == name).sum(), np.abs(pr.lam[groups == name]).max(), r))
    told = tuple(n for n, r in zip(names, res) if r >= 1e-5)
    assert told == K.PINNED, (set(told) ^ set(K.PINNED))


def test_reference_multipliers_push_the_side_of_the_bound_the_row_sits_on():
    """every inequality row with |lam*| > 1e-4 (183 rows): the bound lam* pushes against is finite and the row lies within 1e-3 of it (comp_eps / slip_eps of the
    script: the scale on which KNITRO's interior point calls a row active; measured max 8.4e-4)"""
    pr = K.Problem("m")
    g = pr.g()
    m = (pr.lb != pr.ub) & (np.abs(pr.lam) > 1e-4)
    pushed = np.where(pr.lam > 0, pr.ub, pr.lb)[m]
    dist = np.abs(g[m] - pushed)
    print("%d inequality rows with |lam*| > 1e-4; max distance to the pushed bound %.2e" % (m.sum(), dist[np.isfinite(dist)].max()))
    assert m.sum() == 183
    assert np.isfinite(pushed).all() and dist.max() <= 1e-3


def test_reference_solution_starts_from_the_nominal_stance():
    pr = K.Problem("m")
    assert np.abs(pr.U[:12, 0] - lc("kinodyn").c_init_of(pr.X[:6, 0])).max() <= 1e-15


def test_generate_solver_solution_is_feasible_but_not_a_pin():
    """generate_solver/prevSoln.mat (tag g; the producing script stops at feastol 1e-4 / 4 s wall clock): inside kd.bounds to 5e-5 under both forms of the lateral
    kinematic box, stationarity residual 3.1e-3 -- recorded so that nobody takes the file for a pin"""
    for y0 in (0.10, 0.125):
        pr = K.Problem("g", kin_box_y0=y0)
        g = pr.g()
        viol = np.maximum(np.maximum(pr.lb - g, g - pr.ub), 0.0)
        du = pr.stationarity(pr.lam)[0]
        print("tag g, kin_box_y0 %.3f: primal %.3e (row %d), stationarity %.3e" % (y0, viol.max(), int(np.argmax(viol)), du))
        assert viol.max() <= 5e-5
        assert 1e-4 <= du <= 1e-2


def test_casadi_face_at_the_reference_solution_emulated():
    """(x*, lam*), lam_f = 1 through landing_kinodyn_casadi_eval_host at N = 20: g (1e-11), grad_gamma_x (1e-9, and <= 1e-6: the kernels call the reference's solution
    stationary), the CCS Jacobian scattered dense (grad f + J' lam* <= 1e-6, >= 100 x that with -lam*), lbg / ubg from p bit-equal to kd.bounds"""
    L = _emu_lib()
    K.casadi_face_at_reference(lc("rbd").Rbd(L), "emulation")
    L.close()


def test_hessian_at_the_reference_solution_emulated():
    """landing_kinodyn_nlp_hess with lam* at x* (active contact / complementarity rows, multipliers of a real solve) against central differences of the oracle's
    complex-step gradient: 12 columns -- one of X, jpos, c, f of intervals 1, 9 and 19.  Measured worst error / (1e-6 relative): see the printed line."""
    L = _emu_lib()
    K.hessian_at_reference(lc("rbd").Rbd(L), "cpu", K.hessian_columns(), "emulation")
    L.close()


def test_warm_resolve_from_the_reference_solution_emulated():
    """the solver kernel (landing_kinodyn_solve_batch_host, warm preset) started from the reference's x* through tests/emu: converges again within the preset's
    max_iter to a KKT point <= 1e-6 under the oracle, f <= 1e-7.  Measured: 4 iterations, |x - x*|_inf 1.26e-2 (f* = 0 is a continuum)."""
    from oracle import kinodyn_oracle as ko
    kd = lc("kinodyn")
    mass, Ib, Ibi = K.consts()
    def certify(x, lam, lb, ub, cost, dt, mu):
        gf = np.array([kd.terminal_cost(x[b], N, cost[b][12:], cost[b][:12])[1] for b in range(x.shape[0])])
        return ko.kkt_batch(x, lam, N, dt, mass, Ib, Ibi, mu, lb, ub, gf)
    L = _emu_lib()
    K.warm_resolve_from_reference(lc("rbd").Rbd(L), certify, "emulation")
    L.close()
