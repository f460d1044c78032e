"""An independent reference for ONE Newton step INSIDE the feasibility phase of the two interior-point solvers (test helper: numpy / scipy only; the SRBM
pieces come from oracle.oracle.Oracle, the kinodynamic ones from tests/kd_newton_reference.py).

Inside the phase the solvers take primal-dual Newton steps of the barrier problem of the ELASTIC problem (include/landing_nlp.h, ipm_core.hpp):

    min  rho sum (n + q) - mu sum log(a n b q)     s.t.  g_E(x) = lb_E,   g_I(x) - s = 0,     a = s - lb + n,   b = ub + q - s

with multipliers y (rows), zL / wn (of a >= 0, n >= 0) and zU / wp (of b >= 0, q >= 0).  The kernels eliminate (dn, dzL, dwn, dq, dzU, dwp) row by row by a
closed formula (el_step / el_point_side: sigma = z / D, D = a + z n / w) and run the condensed system through their Riccati recursion.  This module states
the step as it stands -- ONE sparse unsymmetric system in all unknowns, no elimination:

    (W + D_reg) dx + J' y_new                    = -gf              W = sum_r y_r hess g_r: no objective (factor 0, the constant running-cost Hessian dropped)
    J_E dx                                       = -(g_E - lb_E)    equality rows stay hard
    J_I dx - ds                                  = -(g_I - s)
    -y_new,I - dzL + dzU                         = zL - zU          stationarity in s:  y = zU - zL
    zL (ds + dn) + a dzL = mu - a zL      wn dn + n dwn = mu - n wn      dzL + dwn = rho - zL - wn          per finite lower bound
    zU (dq - ds) + b dzU = mu - b zU      wp dq + q dwp = mu - q wp      dzU + dwp = rho - zU - wp          per finite upper bound

factorised by scipy.sparse.linalg.splu and refined with residuals accumulated in np.longdouble over the COO triplets, exactly as
newton_reference.solve_assembled does.  gf is zero for the SRBM solver; the kinodynamic caller passes the terms of the prescribed step of its fixed variables.

Yardsticks (newton_reference's: per quantity, scaled by max(1, |ref|_inf)): e_aug = forward error of the UNREFINED fp64 LU solve of this full system; e_cond = that
of the system condensed NUMERICALLY -- every row's 3 x 3 block [[z, a, 0], [w, 0, n], [0, 1, 1]] inverted by LAPACK (a Schur complement of the row blocks, not the
z / D formula), which gives y_new,I = bar + sigma ds and the condensed matrix [W + D_reg + J_I' Sigma J_I, J_E'; J_E, 0] of newton_reference.condensed.
The same 3 x 3 solves give every eliminated direction's linear dependence on ds (d dn / d ds, ...), which the update checks propagate the bound of ds through.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import newton_reference as nr

LD = np.longdouble
EPS = np.finfo(float).eps
SIDE_NAMES = {"L": ("dn", "dzL", "dwn"), "U": ("dq", "dzU", "dwp")}


def init_rows(g, lb, ub, mu0, rho, first_row):
    """el_init_row (ipm_core.hpp) restated over the rows >= first_row: the entry state of the phase from the row values g.
    Returns dict(s, en, ep, zL, zU, wn, wp, y): zero on every other row and on equality rows (their y = 0)."""
    ng = len(g)
    out = {k: np.zeros(ng) for k in ("s", "en", "ep", "zL", "zU", "wn", "wp", "y")}
    for r in range(first_row, ng):
        if lb[r] == ub[r]:
            continue
        out["s"][r] = g[r]
        if lb[r] > -np.inf:
            v = lb[r] - g[r]
            n0 = max(v, 0.0) + max(1e-2, 0.1 * abs(v))
            out["en"][r] = n0; out["zL"][r] = min(mu0 / (g[r] - lb[r] + n0), 0.5 * rho); out["wn"][r] = rho - out["zL"][r]
        if ub[r] < np.inf:
            v = g[r] - ub[r]
            q0 = max(v, 0.0) + max(1e-2, 0.1 * abs(v))
            out["ep"][r] = q0; out["zU"][r] = min(mu0 / (ub[r] + q0 - g[r]), 0.5 * rho); out["wp"][r] = rho - out["zU"][r]
        out["y"][r] = out["zU"][r] - out["zL"][r]
    return out


def srbm_core(O, p, st, dreg):
    """the NLP's pieces at st = dict(x, y) over the free variables 12.. and the rows 12..: J, W (objective factor 0), the row values and bounds"""
    x = np.asarray(st["x"], float); p = np.ascontiguousarray(p, float)
    nx, ng = O.nx, O.ng
    lb, ub = O.bounds(p)
    g, jv = O.jac_g(x, p)
    J = nr._ccs(*O.pattern_jac(), jv, (ng, nx)).tocsr()[12:, :][:, 12:]
    y = np.array(st["y"], float); y[:12] = 0.0
    if O.form.run_cost:
        Hu = nr._ccs(*O.pattern_hess_rc(), O.hess_l_rc(x, p, 0.0, y), (nx, nx))
    else:
        Hu = nr._ccs(*O.pattern_hess(), O.hess_l(x, p, 0.0, y), (nx, nx))
    H = (Hu + sp.triu(Hu, 1).T).tocsr()[12:, :][:, 12:]
    return dict(J=J, H=H, gf=np.zeros(nx - 12), g=g[12:], lb=lb[12:], ub=ub[12:], D=np.asarray(dreg, float)[12:], n=nx - 12, m=ng - 12)


def _sides(core, row, mu, rho):
    """per side the rows (positions among the system's rows), distance, violation variable, multipliers, right-hand sides and the 3 x 3 blocks' solves"""
    lb, ub = core["lb"], core["ub"]
    ineq = lb != ub
    out = {}
    for side, bound, var, z, w, sd in (("L", lb, "en", "zL", "wn", 1.0), ("U", ub, "ep", "zU", "wp", -1.0)):
        rows = np.nonzero(ineq & np.isfinite(bound))[0]
        s, v, zz, ww = (np.asarray(row[k], float)[rows] for k in ("s", var, z, w))
        dist = (s - bound[rows] + v) if side == "L" else (bound[rows] + v - s)
        A = np.zeros((len(rows), 3, 3))      # unknowns (dv, dz, dw)
        A[:, 0, 0] = zz; A[:, 0, 1] = dist; A[:, 1, 0] = ww; A[:, 1, 2] = v; A[:, 2, 1] = 1.0; A[:, 2, 2] = 1.0
        r = np.stack([mu - dist * zz, mu - v * ww, rho - zz - ww], axis=1)
        e = np.zeros((len(rows), 3)); e[:, 0] = sd * zz      # the column of ds
        if len(rows):
            c = np.linalg.solve(A, r[:, :, None])[:, :, 0]; k = -np.linalg.solve(A, e[:, :, None])[:, :, 0]      # (dv, dz, dw) = c + k ds
        else:
            c = np.zeros((0, 3)); k = np.zeros((0, 3))
        out[side] = dict(rows=rows, dist=dist, v=v, z=zz, w=ww, r=r, sd=sd, c=c, k=k)
    return out, ineq


def full_system(core, row, mu, rho):
    """(K, b, index) of the full system; unknowns dx | y_new | ds | dn dzL dwn | dq dzU dwp"""
    n, m = core["n"], core["m"]
    sides, ineq = _sides(core, row, mu, rho)
    I = np.nonzero(ineq)[0]; mI = len(I)
    posI = -np.ones(m, int); posI[I] = np.arange(mI)
    res = np.where(ineq, core["g"] - np.asarray(row["s"], float), core["g"] - core["lb"])
    PI = sp.csr_matrix((np.ones(mI), (np.arange(mI), I)), shape=(mI, m))
    L, U = sides["L"], sides["U"]
    mL, mU = len(L["rows"]), len(U["rows"])
    SL = sp.csr_matrix((np.ones(mL), (np.arange(mL), posI[L["rows"]])), shape=(mL, mI))
    SU = sp.csr_matrix((np.ones(mU), (np.arange(mU), posI[U["rows"]])), shape=(mU, mI))
    dg = sp.diags
    IL, IU = sp.identity(mL), sp.identity(mU)
    K = sp.bmat([
        [core["H"] + dg(core["D"]), core["J"].T, None, None, None, None, None, None, None],
        [core["J"], None, -PI.T, None, None, None, None, None, None],
        [None, -PI, None, None, -SL.T, None, None, SU.T, None],
        [None, None, dg(L["z"]) @ SL, dg(L["z"]), dg(L["dist"]), None, None, None, None],
        [None, None, None, dg(L["w"]), None, dg(L["v"]), None, None, None],
        [None, None, None, None, IL, IL, None, None, None],
        [None, None, -(dg(U["z"]) @ SU), None, None, None, dg(U["z"]), dg(U["dist"]), None],
        [None, None, None, None, None, None, dg(U["w"]), None, dg(U["v"])],
        [None, None, None, None, None, None, None, IU, IU]], format="csc")
    zL = np.asarray(row["zL"], float)[I]; zU = np.asarray(row["zU"], float)[I]
    b = np.concatenate([-core["gf"], -res, zL - zU, L["r"][:, 0], L["r"][:, 1], L["r"][:, 2], U["r"][:, 0], U["r"][:, 1], U["r"][:, 2]])
    sizes = [n, m, mI, mL, mL, mL, mU, mU, mU]
    off = np.concatenate([[0], np.cumsum(sizes)])
    index = {k: slice(int(off[i]), int(off[i + 1])) for i, k in enumerate(("dx", "y", "ds", "dn", "dzL", "dwn", "dq", "dzU", "dwp"))}
    return K, b, index, sides, ineq, res


def solve_core(core, row, mu, rho, refine=3):
    """The refined step of the elastic problem at the row state row = dict(s, en, ep, zL, wn, zU, wp) (arrays over the system's rows).  Returns a dict in the form of
    newton_reference.solve_assembled -- q = (dx, ds of the inequality rows, y_new of the equality rows), e_aug, e_cond, res, a (the numerically condensed pieces),
    K / b (newton_reference.augmented(a): what backward_error() takes) -- plus, per side "L" / "U": rows, the refined directions dv / dz / dw, their slopes k
    against ds ([:, 0..2] for dv, dz, dw), and the side's state (dist, v, z, w)."""
    n, m = core["n"], core["m"]
    K, b, ix, sides, ineq, res = full_system(core, row, mu, rho)
    lu = spla.splu(K)
    z0 = lu.solve(b)
    coo = K.tocoo()
    z = np.asarray(z0, LD)
    for _ in range(refine):
        z = z + lu.solve(nr._res_ld(coo, z, b).astype(float)).astype(LD)
    r = nr._res_ld(coo, z, b)
    rel = float(np.max(np.abs(r)) / max(float(np.max(np.abs(b))), 1e-300))
    z = z.astype(float)
    # the numerically condensed pieces, in newton_reference's form
    eq = ~ineq
    sig = np.zeros(m); bar = np.zeros(m)
    L, U = sides["L"], sides["U"]
    np.add.at(sig, L["rows"], -L["sd"] * L["k"][:, 1]); np.add.at(sig, U["rows"], -U["sd"] * U["k"][:, 1])      # dz = c - sd sigma ds
    np.add.at(bar, L["rows"], -(L["z"] + L["c"][:, 1])); np.add.at(bar, U["rows"], U["z"] + U["c"][:, 1])
    a = dict(J=core["J"], H=core["H"], gf=core["gf"], sig=sig, bar=bar, res=res, ineq=ineq, eq=eq, D=core["D"], n=n, m=m)
    ref = nr._quantities(a, z[ix["dx"]], z[ix["y"]])
    q0 = nr._quantities(a, z0[ix["dx"]], z0[ix["y"]])
    Kc, bc, I, E, JI, sg = nr.condensed(a)
    zc = spla.splu(Kc).solve(bc)
    qc = (zc[:n], JI @ zc[:n] + res[I], zc[n:])
    names = ("dx", "ds", "y")
    e_aug = {k: float(np.max(np.abs(u - v))) / nr._scale(v) if len(v) else 0.0 for k, u, v in zip(names, q0, ref)}
    e_cond = {k: float(np.max(np.abs(u - v))) / nr._scale(v) if len(v) else 0.0 for k, u, v in zip(names, qc, ref)}
    Ka, ba = nr.augmented(a)
    out = dict(q=ref, z=np.concatenate([z[ix["dx"]], z[ix["y"]]]), e_aug=e_aug, e_cond=e_cond, res=rel, K=Ka, b=ba, a=a)
    for side, S in sides.items():
        nv, nz, nw = SIDE_NAMES[side]
        out[side] = dict(rows=S["rows"], dv=z[ix[nv]], dz=z[ix[nz]], dw=z[ix[nw]], k=S["k"], dist=S["dist"], v=S["v"], z=S["z"], w=S["w"], sd=S["sd"])
    return out


def solve_step(O, p, st, row, mu, rho, dreg, refine=3):
    """SRBM: refined phase step at st = dict(x, y) with the row state `row` (arrays over ng).  Returns newton_reference.scatter()'s dict (dx [nx], ds [ng], y_new [ng],
    ineq / eq, e_aug, e_cond, res, K, b, a, free, rows) plus the sides "L" / "U" of solve_core with `rows` as indices into g."""
    core = srbm_core(O, p, st, dreg)
    sol = solve_core(core, {k: np.asarray(v, float)[12:] for k, v in row.items()}, mu, rho, refine)
    sides = {s: sol.pop(s) for s in ("L", "U")}
    out = nr.scatter(sol, O.nx, O.ng, np.arange(12, O.nx), np.arange(12, O.ng))
    for s, S in sides.items():
        S["rows"] = S["rows"] + 12
        out[s] = S
    return out


def kd_solve_step(pr, st, row, mu, rho, dreg, J, H, refine=3):
    """Kinodynamic refinement: refined phase step at st = dict(x, y) with the row state `row` (arrays over ng); J [ng, nx] and H [nx, nx] = Hessian of y' g as
    kd_newton_reference.solve_step takes them (no objective is added: the phase has none).  The fixed variables take their prescribed step d0, whose terms go to the
    right-hand sides.  Returns the dict of solve_step above (dx of the fixed variables = d0)."""
    import kd_newton_reference as kr
    N = pr.N
    free, fixed, rows = kr.free_index(N), kr.fixed_index(N), np.arange(24, pr.ng)
    assert np.array_equal(kr.row_masks(pr)[1][rows], (pr.lb == pr.ub)[rows])
    x = np.asarray(st["x"], float)
    Jr = sp.csr_matrix(J)[rows]; Hf = sp.csr_matrix(H)
    d0 = np.concatenate([pr.lb[0:12] - x[0:12], pr.lb[12:24] - x[pr.oU:pr.oU + 12]])
    core = dict(J=Jr[:, free], H=Hf[free][:, free], gf=Hf[free][:, fixed] @ d0, g=pr.g(x)[rows] + Jr[:, fixed] @ d0, lb=pr.lb[rows], ub=pr.ub[rows],
                D=np.asarray(dreg, float)[free], n=len(free), m=len(rows))
    sol = solve_core(core, {k: np.asarray(v, float)[rows] for k, v in row.items()}, mu, rho, refine)
    sides = {s: sol.pop(s) for s in ("L", "U")}
    out = nr.scatter(sol, pr.nx, pr.ng, free, rows)
    out["dx"][fixed] = d0
    for s, S in sides.items():
        S["rows"] = S["rows"] + 24
        out[s] = S
    return out


def row_algebra_dense(sd, a, n, z, w, mu, rho, ds):
    """ONE side: (values, term sums, condition sums).  values: dz, dw, dn, da and the side's sigma / rho from a dense solve of its three equations in np.longdouble:
    what the unit check of el_step / el_point_side holds the kernel's closed formulas against.  term sums: the sum of the absolute terms of each output's closed formula
    (the project's yardstick for a formula: its tolerance).  condition sums: |A^-1| |r| of the dense solve -- what a backward-stable 3 x 3 solve would be held to;
    reported only (the closed formula divides by w first and is not backward stable at states with w << z, which the unit check visits and the solvers do not)."""
    A = np.array([[z, a, 0.0], [w, 0.0, n], [0.0, 1.0, 1.0]], LD)
    r = np.array([mu - a * z - sd * z * ds, mu - n * w, rho - z - w], LD)
    rabs = np.array([abs(mu) + abs(a * z) + abs(z * ds), abs(mu) + abs(n * w), abs(rho) + abs(z) + abs(w)], LD)
    # Cramer / adjugate in extended precision (a 3 x 3 system: no LAPACK routine takes np.longdouble)
    det = A[0, 0] * (A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1]) - A[0, 1] * (A[1, 0] * A[2, 2] - A[1, 2] * A[2, 0]) + A[0, 2] * (A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0])
    adj = np.empty((3, 3), LD)
    for i in range(3):
        for j in range(3):
            mnr = np.delete(np.delete(A, j, axis=0), i, axis=1)
            adj[i, j] = (-1) ** (i + j) * (mnr[0, 0] * mnr[1, 1] - mnr[0, 1] * mnr[1, 0])
    Ai = adj / det
    u = Ai @ r; ua = np.abs(Ai) @ rabs
    dn, dz, dw = u
    # the side's part of Sigma and rho in the condensed row: dz = c - sd sigma ds, rho = -sd (z + c)
    r0 = np.array([mu - a * z, mu - n * w, rho - z - w], LD); r0abs = np.array([abs(mu) + abs(a * z), abs(mu) + abs(n * w), abs(rho) + abs(z) + abs(w)], LD)
    sig = (Ai @ np.array([z, 0.0, 0.0], LD))[1]; c = (Ai @ r0)[1]
    val = dict(dz=dz, dw=dw, dn=dn, da=LD(sd) * LD(ds) + dn, sig=sig, rho=-LD(sd) * (LD(z) + c))
    cond = dict(dz=ua[1], dw=ua[2], dn=ua[0], da=abs(LD(ds)) + ua[0], sig=abs(sig), rho=abs(LD(z)) + (np.abs(Ai) @ r0abs)[1])
    # the sums of the absolute terms of the kernel's closed formulas (ipm_core.hpp el_step / el_point_side), each output's terms carried into the next:
    #   dz = (mu - a z - z (mu - n w + n rn) / w - sd z ds) / D,  rn = z + w - rho,  D = a + z n / w  (a sum of positive terms)
    #   dw = -dz - rn,   dn = (mu - n w - n dw) / w,   da = sd ds + dn,   sigma = z / D,   rho_row = -sd (z + c),  c = dz at ds = 0
    a_, n_, z_, w_, mu_, ds_ = (abs(LD(v)) for v in (a, n, z, w, mu, ds))
    Trn = z_ + w_ + abs(LD(rho)); D = a_ + z_ * n_ / w_
    Tc = (mu_ + a_ * z_ + z_ * (mu_ + n_ * w_ + n_ * Trn) / w_) / D
    Tdz = Tc + z_ * ds_ / D; Tdw = Tdz + Trn; Tdn = (mu_ + n_ * w_ + n_ * Tdw) / w_
    mag = dict(dz=Tdz, dw=Tdw, dn=Tdn, da=ds_ + Tdn, sig=abs(sig), rho=z_ + Tc)
    return val, mag, cond
