"""TEST INFRASTRUCTURE shared by tests/test_kd_multipliers_cpu.py and tests/test_gpu_kd_multipliers.py: the reference's own KNITRO solution AND
multipliers of the production kinodynamic refinement problem (tests/golden/n1_kinodyn_multipliers.npz, tag m = main_scripts/prevSoln.mat:
X_star, U_star, jpos_star, lam_g_star [2844], landing_optimization.m:386,395; written by tests/make_golden_n1.py) posed as the project poses that
problem -- production grid ko.REFERENCE_DT, mu 0.75, kd.QN_DEFAULT, kd.Q_TERM_REF, kd.bounds at its defaults -- and the checks of the kernels at that
point that run both on the host emulation and on the device."""
import os

import numpy as np

from conftest import GOLDEN, lc

N = 20
KKT_TOL = 1e-6                       # the tolerance the project's own solutions are certified to (tests/test_gpu_kd_solver.py)
MU = 0.75

# the 27 row groups of the NLP in the order of kd.bounds; PINNED: negating the reference's multipliers of that group alone lifts the
# stationarity residual from 3e-7 to >= 1e-5; UNPINNED: the reference's multipliers of the group are <= ~1e-5 at this solution, so its sign and
# position are pinned by feasibility only
PINNED = ("q_init", "qd_init", "defects", "f_z", "c_z", "lcp", "slip_upper", "slip_lower", "kin_box_x", "kin_box_y", "kin_box_z", "leg_length",
          "friction_0", "friction_1", "friction_2", "friction_3", "z_min", "fk_lower", "fk_upper")
UNPINNED = ("c_init", "q_term_lower", "q_term_upper", "qd_term_lower", "qd_term_upper", "leg_torque", "jpos_lower", "jpos_upper")


def consts():
    mass, Ib, Ibi = lc("constants").robot_constants()
    return mass, np.asarray(Ib), np.asarray(Ibi)


def fixture(tag):
    with np.load(os.path.join(GOLDEN, "n1_kinodyn_multipliers.npz")) as d:
        return d["X_" + tag], d["U_" + tag], d["J_" + tag], d["lam_" + tag]


def row_groups(n=N):
    """group name of every row, walking the layout of kd.bounds (landing-controller_amd/kinodyn.py); checked against what kd.bounds writes where its
    arguments can tell the groups apart (every argument gets a value of its own)"""
    kd = lc("kinodyn")
    names = []
    names += ["q_init"] * 6 + ["qd_init"] * 6 + ["c_init"] * 12 + ["q_term_lower"] * 6 + ["q_term_upper"] * 6 + ["qd_term_lower"] * 6 + ["qd_term_upper"] * 6
    for k in range(n):
        last = k == n - 1
        names += ["defects"] * 12 + ["f_z"] * 4
        for l in range(4):
            names += ["c_z", "lcp"]
            if not last:
                names += ["slip_upper"] * 3 + ["slip_lower"] * 3
            names += ["kin_box_x", "kin_box_y", "kin_box_z", "leg_length"] + ["leg_torque"] * 3
        for s in range(4):
            names += ["friction_%d" % s] * 4
        names += ["z_min"] + ["fk_lower"] * 12 + ["fk_upper"] * 12 + ["jpos_lower"] * 12 + ["jpos_upper"] * 12
    names = np.array(names)
    assert names.size == kd.dims(n)[1] and set(names) == set(PINNED) | set(UNPINNED) and len(PINNED) == 19 and len(UNPINNED) == 8
    v = lambda a, m: a + np.arange(m)
    lb, ub = kd.bounds(n, v(100, 6), v(200, 6), v(300, 12), (1.0, 2.0), q_term_min=v(400, 6), q_term_max=v(500, 6), qd_term_min=v(600, 6), qd_term_max=v(700, 6),
                       z_min=800.0, l_leg_max=30.0, jpos_min=v(1000, 12), jpos_max=v(1100, 12), tau_max=v(1200, 3), comp_eps=1300.0, slip_eps=1400.0, fk_band=1500.0, kin_box_y0=0.5)
    inf = np.inf
    sig = {"q_init": (100, 105, 100, 105), "qd_init": (200, 205, 200, 205), "c_init": (300, 311, 300, 311), "q_term_lower": (400, 405, inf, inf), "q_term_upper": (-inf, -inf, 500, 505),
           "qd_term_lower": (600, 605, inf, inf), "qd_term_upper": (-inf, -inf, 700, 705), "defects": (0, 0, 0, 0), "f_z": (0, 0, inf, inf), "c_z": (0, 0, inf, inf),
           "lcp": (-inf, -inf, 1300, 1300), "slip_upper": (-inf, -inf, 1400, 1400), "slip_lower": (-1400, -1400, inf, inf), "kin_box_x": (-1.125, -1.125, 1.125, 1.125),
           "kin_box_y": (-2.5, -0.05, 0.05, 2.5), "kin_box_z": (-0.4, -0.4, -0.075, -0.075), "leg_length": (-inf, -inf, 900, 900), "leg_torque": (-1202, -1200, 1200, 1202),
           "friction_0": (-inf, -inf, 0, 0), "friction_1": (-inf, -inf, 0, 0), "friction_2": (-inf, -inf, 0, 0), "friction_3": (-inf, -inf, 0, 0), "z_min": (800, 800, inf, inf),
           "fk_lower": (-1500, -1500, inf, inf), "fk_upper": (-inf, -inf, 1500, 1500), "jpos_lower": (1000, 1011, inf, inf), "jpos_upper": (-inf, -inf, 1100, 1111)}
    for name, want in sig.items():
        m = names == name
        assert (lb[m].min(), lb[m].max(), ub[m].min(), ub[m].max()) == want, (name, lb[m].min(), lb[m].max(), ub[m].min(), ub[m].max())
    return names


class Problem:
    """(x*, lam*) of a tag of the fixture with the project's production setting around it"""

    def __init__(self, tag="m", kin_box_y0=0.10):
        from oracle import kinodyn_oracle as ko
        kd = lc("kinodyn")
        self.X, self.U, self.J, self.lam = fixture(tag)
        assert self.X.shape == (12, N + 1) and self.U.shape == (24, N) and self.J.shape == (12, N) and self.lam.shape == (ko.nlp_dims(N)[1],)
        self.x = kd.pack_x(self.X, self.U, self.J)
        self.q_init, self.qd_init = self.X[:6, 0].copy(), self.X[6:, 0].copy()
        self.c_init = kd.c_init_of(self.q_init)
        self.kin_box = kd.kin_box_of(self.q_init[3:6], self.qd_init[3:6])
        self.lb, self.ub = kd.bounds(N, self.q_init, self.qd_init, self.c_init, self.kin_box, kin_box_y0=kin_box_y0)
        self.dt = ko.REFERENCE_DT.copy()
        self.cost = np.concatenate([kd.QN_DEFAULT, kd.Q_TERM_REF, np.zeros(6)]).astype(float)

    def grad_f(self, x=None, z_ref=None):
        kd = lc("kinodyn")
        ref = self.cost[12:].copy()
        if z_ref is not None:
            ref[2] = z_ref
        return kd.terminal_cost(self.x if x is None else x, N, ref, self.cost[:12])

    def g(self, dt=None, mu=MU):
        from oracle import kinodyn_oracle as ko
        mass, Ib, Ibi = consts()
        return ko.nlp_g(self.x, N, self.dt if dt is None else dt, mass, Ib, Ibi, mu)

    def stationarity(self, lams, dt=None, mu=MU, z_ref=None):
        """|grad f + J' lam|_inf at x* for every row of lams [B, ng] (complex-step Jacobian of the oracle)"""
        from oracle import kinodyn_oracle as ko
        mass, Ib, Ibi = consts()
        lams = np.atleast_2d(lams); B = lams.shape[0]
        gf = self.grad_f(z_ref=z_ref)[1]
        r = ko.grad_lagrangian_batch(np.repeat(self.x[None], B, axis=0), lams, N, self.dt if dt is None else dt, mass, Ib, Ibi, mu, np.repeat(gf[None], B, axis=0))
        return np.abs(r).max(axis=1)

    def knitro_params(self):
        """p of the CasADi-external face for this instance (the script's values; Xref matters in its last column only, :83-86)"""
        kd = lc("kinodyn")
        mass, Ib, Ibi = consts()
        Xref = np.zeros((12, N + 1))
        for i in range(6):
            Xref[i] = np.linspace(self.q_init[i], self.cost[12 + i], N + 1); Xref[6 + i] = np.linspace(self.qd_init[i], 0.0, N + 1)
        return kd.pack_params_knitro(N, Xref=Xref, dt=self.dt, q_init=self.q_init, qd_init=self.qd_init, c_init=self.c_init, jpos_min=kd.JPOS_MIN, jpos_max=kd.JPOS_MAX,
                                     q_term_min=[-10, -10, 0.15, -0.1, -0.1, -10], q_term_max=[10, 10, 5, 0.1, 0.1, 10], qd_term_min=[-10, -10, -10, -.5, -.5, -.5],
                                     qd_term_max=[10, 10, 10, .5, .5, .5], q_min=[-10, -10, 0.075, -10, -10, -10], QN=self.cost[:12], mu=MU, l_leg_max=0.4, mass=mass, Ib=Ib,
                                     Ib_inv=Ibi, kin_box=self.kin_box)


def scatter_ccs(colind, rows, vals, shape):
    A = np.zeros(shape)
    for c in range(shape[1]):
        A[rows[colind[c]:colind[c + 1]], c] = vals[colind[c]:colind[c + 1]]
    return A


def check_face_outputs(pr, g, ggx, J, lb, ub, label):
    """the outputs of the CasADi-external face at (x*, lam*) with lam_f = 1 (g [ng], grad_gamma_x [nx], the Jacobian scattered dense [ng, nx], lbg / ubg from p)
    against the oracle and against the reference's multipliers"""
    from oracle import kinodyn_oracle as ko
    mass, Ib, Ibi = consts()
    nx, ng = ko.nlp_dims(N)
    f, gf = pr.grad_f()
    eg = np.abs(g - pr.g()).max()
    ref = ko.grad_lagrangian_batch(pr.x[None], pr.lam[None], N, pr.dt, mass, Ib, Ibi, MU, gf[None])[0]
    ex = np.abs(ggx - ref).max()
    du, du_neg = np.abs(gf + J.T @ pr.lam).max(), np.abs(gf - J.T @ pr.lam).max()
    print("%s: |g - oracle| %.2e; |ggx - oracle| %.2e; max|ggx| %.4e; |grad f + J' lam*| %.4e, with -lam* %.4e (x %.0f)" % (label, eg, ex, np.abs(ggx).max(), du, du_neg, du_neg / du))
    assert eg <= 1e-11
    assert ex <= 1e-9 * max(1.0, np.abs(ggx).max())
    assert np.abs(ggx).max() <= KKT_TOL
    assert du <= KKT_TOL and du_neg >= 100.0 * du
    assert np.array_equal(lb, pr.lb) and np.array_equal(ub, pr.ub)


def casadi_face_at_reference(R, label):
    """(x*, lam*) with lam_f = 1 through rbd.Rbd.kinodyn_casadi_eval (landing_kinodyn_casadi_eval_host) and kinodyn_casadi_bounds"""
    pr = Problem("m")
    nx, ng = R.kinodyn_nlp_dims(N)
    p = pr.knitro_params()
    r = R.kinodyn_casadi_eval(N, pr.x, p, 1.0, pr.lam, want=("f", "g", "grad_f", "jac", "ggx"))
    f, gf = pr.grad_f()
    assert abs(r["f"] - f) <= 1e-15 and np.array_equal(r["grad_f"], gf)
    jc, jr = R.kinodyn_casadi_pattern(N, 0)
    lb, ub = R.kinodyn_casadi_bounds(N, p)
    check_face_outputs(pr, r["g"], r["ggx"], scatter_ccs(jc, jr, r["jac"], (ng, nx)), lb, ub, label)


# ---- Hessian of lam*' g at x* -------------------------------------------------------------------------------------------------------------
HESS_H = 1e-5
# The reference for a column is a central difference (step h = 1e-5) of the oracle's complex-step J' lam*, which is exact to rounding.  With |lam*| <= 0.02 and
# forces of ~1e2 N the entries of J' lam* are sums of a few terms of size <= ~2 and the third derivatives of lam*' g are <= ~2, so a column is good to about
# 1e-16 * 4 / (2 h) + h^2 / 6 * 2 ~ 5e-11 ABSOLUTE.  The entries of this Hessian are small (largest ~5e-4: lam* is small), so the tolerance is taken relative to
# the largest entry S of the differenced columns, not to max(1, .): error <= 1e-6 S ~ 5e-10, ten times the estimate above, ten times below the 1e-5 of
# tests/test_n1_rows.py::_hess_check's oracle differences, and 1e-6 of the quantity itself.
HESS_TOL = 1e-6


def hessian_columns(n_int=(1, 9, N - 1)):
    """x indices of one column from each of X, jpos, c, f of an early, a middle and the last interval (12 columns): a rotation angle, a knee joint, a foot height
    / a foot x, a vertical / a horizontal force"""
    from oracle import kinodyn_oracle as ko
    cols = []
    for i, k in enumerate(n_int):
        for j in ((4, 38, 14, 26), (3, 41, 12, 24), (7, 37, 17, 35))[i % 3]:
            cols.append(ko.w_index(N, k, j))
    return cols


def hessian_at_reference(R, dev, cols, label, chunk=64):
    """rbd.Rbd.kinodyn_nlp_hess with lam* at x* (blocks [N, 72, 72] summed into the [nx, nx] Hessian of lam*' g; the boundary rows are linear) against central
    differences of the oracle's complex-step J' lam*, column by column.  Returns the worst error / tolerance ratio."""
    import torch
    from oracle import kinodyn_oracle as ko
    mass, Ib, Ibi = consts()
    pr = Problem("m")
    nx, ng = ko.nlp_dims(N)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    dx, dl = t(pr.x[None]), t(pr.lam[None])
    Hb = torch.zeros(1, N, 72, 72, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream if dev == "cuda" else 0
    R.kinodyn_nlp_hess(1, N, dx.data_ptr(), pr.dt, mass, Ib, Ibi, MU, dl.data_ptr(), Hb.data_ptr(), st)
    if dev == "cuda":
        torch.cuda.synchronize()
    Hb = Hb.cpu().numpy()[0]
    assert np.array_equal(Hb, Hb.transpose(0, 2, 1)) and np.isfinite(Hb).all()
    wm = ko._w_map(N)
    H = np.zeros((nx, nx))
    for k in range(N):
        ok = wm[k] >= 0
        assert (Hb[k][~ok] == 0.0).all() and (Hb[k][:, ~ok] == 0.0).all()
        np.add.at(H, (wm[k][ok][:, None], wm[k][ok][None, :]), Hb[k][np.ix_(ok, ok)])
    cols = list(cols)
    zero = np.zeros((1, nx))
    ref = np.zeros((nx, len(cols)))
    for lo in range(0, len(cols), chunk):
        cc = cols[lo:lo + chunk]
        xp = np.repeat(pr.x[None], 2 * len(cc), axis=0)
        for q, j in enumerate(cc):
            xp[2 * q, j] += HESS_H; xp[2 * q + 1, j] -= HESS_H
        gl = ko.grad_lagrangian_batch(xp, np.repeat(pr.lam[None], 2 * len(cc), axis=0), N, pr.dt, mass, Ib, Ibi, MU, np.repeat(zero, 2 * len(cc), axis=0))
        ref[:, lo:lo + len(cc)] = ((gl[0::2] - gl[1::2]) / (2 * HESS_H)).T
    S = np.abs(ref).max()
    err = np.abs(H[:, cols] - ref).max(axis=0)
    worst, worst_col = err.max() / (HESS_TOL * S), cols[int(np.argmax(err))]
    print("%s: Hessian of lam*' g at x*, %d columns: largest entry S %.3e; worst error %.3e = %.3e x the tolerance 1e-6 S (column %d)" % (label, len(cols), S, err.max(), worst, worst_col))
    assert S > 1e-4                                     # (lam* is not zero: the comparison is not of zeros with zeros)
    assert worst <= 1.0, (worst, worst_col)
    return worst


# ---- the warm re-solve started from the reference's solution ----------------------------------------------------------------------------------
def warm_resolve_from_reference(R, certify, label):
    """landing_kinodyn_solve_batch_host with the warm preset from x0 = x*, the file's own initial state, stance and kd.bounds: status 0 within the preset's
    max_iter, a KKT point <= 1e-6 under the oracle (certify(x, lam, lb, ub, cost, dt, mu) -> [1, 3]) with f <= 1e-7.  The optimum f* = 0 is a continuum, so the
    distance to x* is printed, not asserted.  Returns (iterations, |x - x*|_inf)."""
    kd = lc("kinodyn")
    pr = Problem("m")
    mass, Ib, Ibi = consts()
    lb, ub = kd.bounds(N, pr.q_init, pr.qd_init, pr.U[:12, 0], pr.kin_box)
    w = R.kinodyn_warm_opts()
    s = R.kinodyn_solve_host(N, lb, ub, pr.cost, pr.x, pr.dt, mass, Ib, Ibi, MU, w)
    k = certify(s["x"], s["lam_g"], lb[None], ub[None], pr.cost[None], pr.dt, MU)
    dx = np.abs(s["x"][0] - pr.x).max()
    print("%s: warm re-solve from the reference's x*: status %d, %d iterations (max_iter %d), f %.3e, kkt(oracle) %s, |x - x*|_inf %.3e" % (
        label, s["status"][0], s["iters"][0], w.max_iter, s["f"][0], np.array2string(k[0], precision=3), dx))
    assert s["status"][0] == 0, (s["status"], s["kkt"])
    assert k.max() <= KKT_TOL * 1.0001, k
    assert s["f"][0] <= 1e-7
    assert s["iters"][0] <= w.max_iter
    return int(s["iters"][0]), dx
