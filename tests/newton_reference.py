"""An independent reference for ONE Newton step of the SRBM interior-point solver (test helper: numpy / scipy and oracle.oracle.Oracle only).

The solver kernel condenses the primal-dual system stage by stage and solves it by a Riccati recursion.  This module solves the same step
as one sparse symmetric system in (dx_free, y_new), which shares no code and no structure with the kernel:

    [ H + D_reg   J' ] [ dx    ]   [ -grad f                              ]        S = 0 (equality rows), 1 / sigma (inequality rows)
    [ J          -S  ] [ y_new ] = [ -(g - b)   or   -(g - s) - bar / sigma ]       sigma = zL / (s - lb) + zU / (ub - s)
                                                                                    bar   = mu / (ub - s) - mu / (s - lb)

x[0:12] (fixed by rows 0..11) and those rows are left out.  J, H(x, y), grad f come from the oracle; the system is factorised by
scipy.sparse.linalg.splu and refined with residuals accumulated in np.longdouble over the COO triplets.  ds of the inequality rows is
evaluated from the row identity ds = J_I dx + (g - s) in np.longdouble, which equals (y_new - bar) / sigma at the solution and does not divide
by sigma where a bound multiplier has gone to ~1e-10.

THE REGULARISATION IS NOT delta * I.  The kernel adds delta to the diagonal of every stage block, over the stage's state (X_k, c_k) and its
control (f_k, c_{k+1}).  The feet c_1 .. c_{N-1} are the control of one stage and the state of the next: they receive 2 * delta
(include/landing_nlp.h, delta_init).  d_reg() encodes that; d_reg_plain() is the delta * I the tests show to be wrong.

Yardsticks (per quantity, scaled like the kernel's error by max(1, |ref|_inf)): the forward errors of two UNREFINED fp64 sparse LU solves
against the refined solution -- e_aug, of the augmented system above, and e_cond, of the condensed system
[H + D_reg + J_I' Sigma J_I, J_E'; J_E, 0] -- i.e. what an fp64 method of either structure achieves on this very system.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

LD = np.longdouble
TOL_FACTOR = 16.0      # kernel error <= TOL_FACTOR * max(e_aug, e_cond, TOL_FLOOR)
TOL_FLOOR = 1e-15


def foot_twice(N):
    """indices in x of the feet c_1 .. c_{N-1} (U_k = [c_k | f_k] at 12 (N + 1) + 24 k)"""
    return np.concatenate([12 * (N + 1) + 24 * k + np.arange(12) for k in range(1, N)]) if N > 1 else np.zeros(0, int)


def d_reg(N, delta):
    """the kernel's regularisation: delta on every free variable, 2 delta on c_1 .. c_{N-1}"""
    d = np.full(36 * N + 12, float(delta))
    d[foot_twice(N)] *= 2.0
    return d


def d_reg_plain(N, delta):
    return np.full(36 * N + 12, float(delta))


def delta_schedule(opts, n_fact, floor):
    """regularisation of the n_fact-th factorisation of an iteration that starts the schedule afresh (delta_last = 0, as in the first
    iteration): floor, then delta_init (floor = 0) or floor * delta_inc_first, then * delta_inc_first per further failure (ipm_core.hpp)"""
    d = float(floor)
    for _ in range(int(n_fact) - 1):
        d = opts.delta_init if d == 0.0 else d * opts.delta_inc_first
    return d


def effective_opts(opts, run_cost):
    """(mu_init, bound_push, bound_frac) as the solve entry point resolves the automatic (zero) values"""
    mu = opts.mu_init if opts.mu_init > 0.0 else (0.1 if run_cost else 0.5)
    push = opts.bound_push if opts.bound_push > 0.0 else (0.5 if run_cost else 1.0)
    return mu, push, opts.bound_frac


def push_slacks(g, lb, ub, push, frac, first_row):
    """slack initialisation of both solvers (ipm_core.hpp ipm_init_row restated) over the rows >= first_row: slacks of the inequality rows pushed
    into the interior by bound_push / bound_frac, multipliers of finite bounds 1.  Returns (s, zL, zU), zero on every other row."""
    ng = len(g)
    s = np.zeros(ng); zL = np.zeros(ng); zU = np.zeros(ng)
    for r in range(first_row, ng):
        if lb[r] == ub[r]:
            continue
        hL, hU = lb[r] > -np.inf, ub[r] < np.inf
        if hL and hU:
            pl = min(push * max(1.0, abs(lb[r])), frac * (ub[r] - lb[r])); pu = min(push * max(1.0, abs(ub[r])), frac * (ub[r] - lb[r]))
        else:
            pl = push * max(1.0, abs(lb[r]) if hL else 0.0); pu = push * max(1.0, abs(ub[r]) if hU else 0.0)
        v = g[r]
        if hL:
            v = max(v, lb[r] + pl)
        if hU:
            v = min(v, ub[r] - pu)
        s[r] = v; zL[r] = 1.0 if hL else 0.0; zU[r] = 1.0 if hU else 0.0
    return s, zL, zU


def initial_state(O, p, x0, opts):
    """cold start of the solver (ipm_init_row restated): x0 with the initial state taken from p, slacks pushed into the interior by
    bound_push / bound_frac, multipliers of finite bounds 1, y = zU - zL, equality multipliers 0.  Returns dict(x, s, zL, zU, y, mu)."""
    po = O.param_offsets()
    x = np.array(x0, float)
    x[0:6] = p[po["q_init"]:po["q_init"] + 6]; x[6:12] = p[po["qd_init"]:po["qd_init"] + 6]
    mu, push, frac = effective_opts(opts, O.form.run_cost != 0)
    lb, ub = O.bounds(p)
    s, zL, zU = push_slacks(O.g(x, p), lb, ub, push, frac, 12)
    return dict(x=x, s=s, zL=zL, zU=zU, y=zU - zL, mu=mu)


def _ccs(ci, r, v, shape):
    return sp.csc_matrix((np.asarray(v, float), np.asarray(r), np.asarray(ci)), shape=shape)


def _res_ld(coo, z, b):
    """b - K z in extended precision, accumulated over the COO triplets"""
    r = np.asarray(b, LD).copy()
    np.subtract.at(r, coo.row, coo.data.astype(LD) * np.asarray(z, LD)[coo.col])
    return r


def _scale(v):
    return max(1.0, float(np.max(np.abs(v)))) if len(v) else 1.0


def sigma_bar(s, zL, zU, lb, ub, mu, ineq):
    """sigma = zL / (s - lb) + zU / (ub - s) and bar = mu / (ub - s) - mu / (s - lb) of the inequality rows (finite sides only), zero elsewhere"""
    ng = len(s)
    sig = np.zeros(ng); bar = np.zeros(ng)
    with np.errstate(divide="ignore", invalid="ignore"):
        hL = ineq & (lb > -np.inf); hU = ineq & (ub < np.inf)
        sig[hL] += zL[hL] / (s[hL] - lb[hL]); bar[hL] -= mu / (s[hL] - lb[hL])
        sig[hU] += zU[hU] / (ub[hU] - s[hU]); bar[hU] += mu / (ub[hU] - s[hU])
    return sig, bar


def assemble(O, p, st, mu, dreg):
    """the pieces of the step at state st = dict(x, s, zL, zU, y): free variables 12.., rows 12.."""
    x = np.asarray(st["x"], float); p = np.ascontiguousarray(p, float)
    nx, ng = O.nx, O.ng
    lb, ub = O.bounds(p)
    rows = np.arange(ng)
    ineq = (lb != ub) & (rows >= 12); eq = (lb == ub) & (rows >= 12)
    g, jv = O.jac_g(x, p)
    J = _ccs(*O.pattern_jac(), jv, (ng, nx)).tocsr()[12:, :][:, 12:]
    y = np.array(st["y"], float); y[:12] = 0.0      # the rows of the fixed initial state are linear and carry no multiplier inside the iteration
    if O.form.run_cost:
        Hu = _ccs(*O.pattern_hess_rc(), O.hess_l_rc(x, p, 1.0, y), (nx, nx))
    else:
        Hu = _ccs(*O.pattern_hess(), O.hess_l(x, p, 1.0, y), (nx, nx))
    H = (Hu + sp.triu(Hu, 1).T).tocsr()[12:, :][:, 12:]      # the oracle's Hessian is one triangle
    gf = O.grad_f(x, p)[1][12:]
    s, zL, zU = (np.asarray(st[k], float) for k in ("s", "zL", "zU"))
    sig, bar = sigma_bar(s, zL, zU, lb, ub, mu, ineq)
    res = np.where(ineq, g - s, g - lb)      # g - s / g - b
    return dict(J=J, H=H, gf=gf, sig=sig[12:], bar=bar[12:], res=res[12:], ineq=ineq[12:], eq=eq[12:], D=np.asarray(dreg, float)[12:], n=nx - 12, m=ng - 12)


def augmented(a):
    n, m = a["n"], a["m"]
    Sd = np.zeros(m); Sd[a["ineq"]] = 1.0 / a["sig"][a["ineq"]]
    K = sp.bmat([[a["H"] + sp.diags(a["D"]), a["J"].T], [a["J"], -sp.diags(Sd)]], format="csc")
    b = np.concatenate([-a["gf"], -a["res"] - np.where(a["ineq"], a["bar"] * Sd, 0.0)])
    return K, b


def condensed(a):
    n = a["n"]
    I, E = np.nonzero(a["ineq"])[0], np.nonzero(a["eq"])[0]
    JI, JE = a["J"][I], a["J"][E]
    sg = a["sig"][I]
    rho = a["bar"][I] + sg * a["res"][I]
    K = sp.bmat([[a["H"] + sp.diags(a["D"]) + JI.T @ sp.diags(sg) @ JI, JE.T], [JE, None]], format="csc")
    b = np.concatenate([-a["gf"] - JI.T @ rho, -a["res"][E]])
    return K, b, I, E, JI, sg


def _quantities(a, dx, y_new):
    """(dx, ds on inequality rows, y_new on equality rows) from a solution of the augmented system; ds in extended precision"""
    I = np.nonzero(a["ineq"])[0]
    JI = a["J"][I].tocoo()
    ds = np.asarray(a["res"][I], LD).copy()
    np.add.at(ds, JI.row, JI.data.astype(LD) * np.asarray(dx, LD)[JI.col])
    return np.asarray(dx, float), ds.astype(float), np.asarray(y_new, float)[a["eq"]]


def solve_assembled(a, refine=3):
    """The refined step of an assembled system a = dict(J, H, gf, sig, bar, res, ineq, eq, D, n, m) over its free variables and rows (whichever NLP
    it came from).  Returns dict: q = (dx [n], ds of the inequality rows, y_new of the equality rows), z (dx | y_new of all rows), e_aug / e_cond:
    dict(dx, ds, y) of the two yardsticks, res: relative residual of the refined solution, and K, b, a."""
    n, m = a["n"], a["m"]
    K, b = augmented(a)
    lu = spla.splu(K)
    z0 = lu.solve(b)
    coo = K.tocoo()
    z = np.asarray(z0, LD)
    for _ in range(refine):
        z = z + lu.solve(_res_ld(coo, z, b).astype(float)).astype(LD)
    r = _res_ld(coo, z, b)
    rel = float(np.max(np.abs(r)) / max(float(np.max(np.abs(b))), 1e-300))
    z = z.astype(float)
    ref = _quantities(a, z[:n], z[n:])
    # yardstick 1: the same system, unrefined
    q0 = _quantities(a, z0[:n], z0[n:])
    # yardstick 2: the condensed system, unrefined
    Kc, bc, I, E, JI, sg = condensed(a)
    zc = spla.splu(Kc).solve(bc)
    dxc = zc[:n]
    dsc = JI @ dxc + a["res"][I]
    qc = (dxc, dsc, zc[n:])
    names = ("dx", "ds", "y")
    e_aug = {k: float(np.max(np.abs(u - v))) / _scale(v) if len(v) else 0.0 for k, u, v in zip(names, q0, ref)}
    e_cond = {k: float(np.max(np.abs(u - v))) / _scale(v) if len(v) else 0.0 for k, u, v in zip(names, qc, ref)}
    return dict(q=ref, z=z, e_aug=e_aug, e_cond=e_cond, res=rel, K=K, b=b, a=a)


def scatter(sol, nx, ng, free, rows):
    """a solve_assembled() result over the NLP's own index spaces: free / rows = indices in x / g of the system's variables / rows.  Adds
    dx [nx] (0 on the other variables), ds [ng] (inequality rows, 0 elsewhere), y_new [ng] (all rows of the system), ineq / eq (masks over ng)."""
    a = sol["a"]; n = a["n"]
    free = np.asarray(free); rows = np.asarray(rows)
    dx = np.zeros(nx); dx[free] = sol["q"][0]
    ineq = np.zeros(ng, bool); ineq[rows] = a["ineq"]
    eq = np.zeros(ng, bool); eq[rows] = a["eq"]
    ds = np.zeros(ng); ds[ineq] = sol["q"][1]
    y_new = np.zeros(ng); y_new[rows] = sol["z"][n:]
    out = dict(sol); del out["q"], out["z"]
    out.update(dx=dx, ds=ds, y_new=y_new, ineq=ineq, eq=eq, free=free, rows=rows)
    return out


def solve_step(O, p, st, mu, dreg, refine=3):
    """Refined Newton step at st.  Returns dict:
      dx [nx] (dx[0:12] = 0), ds [ng] (inequality rows, 0 elsewhere), y_new [ng] (all rows >= 12), ineq / eq (row masks over ng),
      e_aug / e_cond: dict(dx, ds, y) of the two yardsticks, res: relative residual of the refined solution,
      and what backward_error() needs (K, b, a, free, rows)."""
    nx, ng = O.nx, O.ng
    return scatter(solve_assembled(assemble(O, p, st, mu, dreg), refine), nx, ng, np.arange(12, nx), np.arange(12, ng))


def errors(ref, dx, ds, yn):
    """the kernel's errors against the reference: dict(dx, ds, y), each |kernel - ref|_inf / max(1, |ref|_inf)"""
    out = {}
    for k, u, v in (("dx", dx, ref["dx"]), ("ds", ds[ref["ineq"]], ref["ds"][ref["ineq"]]), ("y", yn[ref["eq"]], ref["y_new"][ref["eq"]])):
        out[k] = float(np.max(np.abs(np.asarray(u, float) - v))) / _scale(v)
    return out


def bounds_of(ref):
    """per quantity: TOL_FACTOR * max(e_aug, e_cond, TOL_FLOOR)"""
    return {k: TOL_FACTOR * max(ref["e_aug"][k], ref["e_cond"][k], TOL_FLOOR) for k in ("dx", "ds", "y")}


def ratios(ref, err):
    """error over max(e_aug, e_cond, TOL_FLOOR): the figure the docstrings and DESIGN.md record (the bound is TOL_FACTOR)"""
    return {k: err[k] / max(ref["e_aug"][k], ref["e_cond"][k], TOL_FLOOR) for k in err}


def backward_error(ref, dx, ds, yn):
    """normwise backward error of the kernel's step in the augmented system (inequality multipliers from its ds: y = sigma ds + bar), with the
    extended-precision residual: |b - K z|_inf / (|K|_inf |z|_inf + |b|_inf).  Reported, never asserted."""
    a = ref["a"]
    y = np.array(np.asarray(yn)[ref["rows"]], float)
    I = a["ineq"]
    y[I] = a["sig"][I] * np.asarray(ds)[ref["rows"]][I] + a["bar"][I]
    z = np.concatenate([np.asarray(dx)[ref["free"]], y])
    K, b = ref["K"], ref["b"]
    r = _res_ld(K.tocoo(), z, b)
    return float(np.max(np.abs(r))) / (float(abs(K).sum(axis=1).max()) * float(np.max(np.abs(z))) + float(np.max(np.abs(b))))


def inertia_dense(ref):
    """(positive, negative, zero) eigenvalue counts of the augmented matrix by a dense LDL' (small horizons only)"""
    import scipy.linalg as sla
    A = ref["K"].toarray()
    _, d, _ = sla.ldl(A)
    pos = neg = zero = 0
    i, nn = 0, d.shape[0]
    while i < nn:
        if i + 1 < nn and d[i + 1, i] != 0.0:
            w = np.linalg.eigvalsh(d[i:i + 2, i:i + 2]); i += 2
        else:
            w = np.array([d[i, i]]); i += 1
        pos += int((w > 0).sum()); neg += int((w < 0).sum()); zero += int((w == 0).sum())
    return pos, neg, zero
