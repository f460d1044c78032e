"""What a certificate of local infeasibility (status LANDING_INFEASIBLE, include/landing_nlp.h) has to satisfy, from plain arrays: test
infrastructure, independent of both solvers (it knows neither kernel, neither workspace, neither row order).

The status claims a KKT point of the ELASTIC problem with positive violation,

    min  rho * sum(n + q)    s.t.   g_r(x) = lb_r                        (rows with lb == ub)
                                    lb_r <= g_r(x) + n_r,  g_r(x) - q_r <= ub_r,  n, q >= 0     (the other rows),

with the multipliers the solvers return: lam = zU - zL (CasADi's sign: > 0 pushes against ub), zL / zU the multipliers of the two elastic
sides.  Stationarity in n and q gives the further multipliers w_n = rho - zL >= 0, w_q = rho - zU >= 0 of n, q >= 0; stationarity in x has
no objective term: J' lam = 0.

THE BOUNDS.  None is fitted to a solver's output; each follows from the stop test the status claims (ipm_core.hpp ipm_decide: pr, du, co <= tol
with |z + w - rho| folded into du).  With the slack s of a row, a = s - lb + n and b = ub + q - s the distances, that test is

    (i) |g - s| <= tol,  |g_r - lb_r| <= tol on equality rows        (pr)
    (ii) |J' lam|_inf <= tol,  |z + w - rho| <= tol per side          (du)
    (iii) a zL <= tol,  n w_n <= tol,  b zU <= tol,  q w_q <= tol     (co)         and  a, b, n, q, z, w >= 0.

  E  equality rows: max |g_r - lb_r| <= tol                                                                                    from (i).
  S  |J' lam|_inf <= tol over ALL of x.  The solvers test the free variables; the multipliers of the rows that fix the initial variables
     are written from stationarity, so those columns are zero up to rounding and are held to the same bound.  The multipliers are of size
     rho = 1e3: the sum sum_r J_ri lam_r carries a rounding error of its own, allowed for by 8 eps max_i sum_r |J_ri lam_r|
     (computed here from |J|' |lam|; 8 = a handful of roundings per term of a sum whose partial sums never exceed that 1-norm).
  B  inequality rows: |lam_r| <= rho + tol  (zL = rho - w_n + (zL + w_n - rho) <= rho + tol by (ii), w_n >= 0; zU likewise; lam = zU - zL with
     both >= 0).  A row without an upper bound has no zU: lam_r <= 0 exactly; without a lower bound lam_r >= 0 exactly.
  V  a row violated by v_r (upper side: g - ub, lower side: lb - g) carries the full price.  Lower side: n = a + lb - s >= lb - s >= v - tol by
     (i), so w_n <= tol / (v - tol) by (iii) and zL >= rho - tol - w_n by (ii):   rho - |lam_r| <= tol + tol / (v_r - tol).
     On a two-sided row the other side is at distance b >= ub - s >= ub - lb + v - tol >= ub - lb, so zU <= tol / (ub - lb) comes off |lam_r|:
     that term is added.  The sign is part of the claim: lam_r -> +rho on the upper side, -rho on the lower side.  Applied above the floor
     v_r > 100 tol, where the bound says something (tol + tol / (99 tol) ~ 1e-2 against rho = 1e3).
  C  a row strictly inside the bound its multiplier pushes against (lam > 0: dist = ub - g > 0; lam < 0: dist = g - lb > 0).  Upper side:
     dist = b - q + (s - g) <= b + tol, zU dist <= b zU + tol zU:                   |lam_r| dist_r <= tol (1 + |lam_r|)
     for a one-sided row (|lam| = zU).  On a two-sided row zU = |lam| + zL and the smaller of zL, zU is at most 2 tol / (ub - lb) (a + b >=
     ub - lb), which adds 2 tol^2 / (ub - lb); the other side's tol / (ub - lb) is added, which covers it.
  P  positive violation: sum_r v_r > feas_cert, and max_r v_r is the kkt[0] the solver reports (to kkt0_atol: the two evaluate the same rows
     in another order of operations).

Every bound carries the suite's factor 1.0001 on its tol part."""
import numpy as np

EPS = np.finfo(float).eps
FACTOR = 1.0001
NAMES = ("E", "S", "B", "V", "C", "P")


def _worst(value, bound, rows):
    """the row with the largest value / bound: (value, bound, row, ok); (0, bound 0, -1, True) over no rows"""
    if len(rows) == 0:
        return dict(value=0.0, bound=0.0, row=-1, ok=True, rows=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0.0, value / bound, np.where(value > 0.0, np.inf, 0.0))
    ratio = np.where(np.isfinite(value), ratio, np.inf)      # (a NaN never passes)
    i = int(np.argmax(ratio))
    return dict(value=float(value[i]), bound=float(bound[i]), row=int(rows[i]), ok=bool(np.isfinite(value[i]) and value[i] <= bound[i]), rows=len(rows))


def certificate_residuals(g, lb, ub, lam, rho, tol, J=None, Jt_lam=None, absJt_abslam=None, feas_cert=1e-4, kkt0=None, kkt0_atol=1e-9):
    """g, lb, ub, lam [ng]: rows, bounds (+-inf where there is none) and returned multipliers at the point; rho = feas_rho, tol = the solver's tol.
    The Jacobian: J [ng, nx] (scipy sparse or dense), or Jt_lam = J' lam [nx] together with absJt_abslam = |J|' |lam| [nx].
    Returns {name: dict(value, bound, row, ok, rows)} for E, S, B, V, C, P: value and bound of the worst row (largest value / bound; row = its
    index, -1 where the residual is not per row; rows = how many rows it was taken over), ok = every row within its bound.
    B also carries `sign` (largest multiplier of the wrong sign on a one-sided row, must be 0) and P `v1` (the 1-norm violation)."""
    g, lb, ub, lam = (np.asarray(a, float) for a in (g, lb, ub, lam))
    assert g.shape == lb.shape == ub.shape == lam.shape and g.ndim == 1 and (lb <= ub).all() and rho > 0.0 and tol > 0.0
    t = tol * FACTOR
    rows = np.arange(len(g))
    eq = lb == ub
    iq = ~eq
    hL, hU = np.isfinite(lb), np.isfinite(ub)
    two = iq & hL & hU
    with np.errstate(invalid="ignore", divide="ignore"):
        other = np.where(two, t / (ub - lb), 0.0)      # the other side of a two-sided row
        vU, vL = np.where(hU, g - ub, -np.inf), np.where(hL, lb - g, -np.inf)
    out = {}
    # E
    out["E"] = _worst(np.abs(g[eq] - lb[eq]), np.full(eq.sum(), t), rows[eq])
    # S
    if J is not None:
        Jl = np.asarray(J.T @ lam).ravel()
        aJ = np.asarray(abs(J).T @ np.abs(lam)).ravel()
    else:
        Jl, aJ = np.asarray(Jt_lam, float).ravel(), np.asarray(absJt_abslam, float).ravel()
    i = int(np.argmax(np.where(np.isfinite(Jl), np.abs(Jl), np.inf)))
    sb = t + 8.0 * EPS * float(aJ.max())
    out["S"] = dict(value=float(abs(Jl[i])), bound=sb, row=i, ok=bool(np.isfinite(Jl).all() and abs(Jl[i]) <= sb), rows=len(Jl), rounding=8.0 * EPS * float(aJ.max()))
    # B
    out["B"] = _worst(np.abs(lam[iq]), np.full(iq.sum(), rho + t), rows[iq])
    sign = np.maximum(np.where(iq & ~hU, lam, 0.0), np.where(iq & ~hL, -lam, 0.0))
    out["B"]["sign"] = float(sign.max()) if len(sign) else 0.0
    if out["B"]["sign"] > 0.0:
        out["B"].update(ok=False, row=int(np.argmax(sign)))
    # V
    v = np.where(iq, np.maximum(np.maximum(vU, vL), 0.0), 0.0)
    side = np.where(vU >= vL, 1.0, -1.0)      # the violated side (a row cannot be violated on both)
    big = iq & (v > 100.0 * tol)
    with np.errstate(invalid="ignore", divide="ignore"):
        vb = t + t / (v - tol) + other
    out["V"] = _worst((rho - side * lam)[big], vb[big], rows[big])
    # C
    with np.errstate(invalid="ignore"):
        dist = np.where(lam > 0.0, ub - g, np.where(lam < 0.0, g - lb, 0.0))
    ins = iq & (lam != 0.0) & np.isfinite(dist) & (dist > 0.0)
    out["C"] = _worst((np.abs(lam) * dist)[ins], (t * (1.0 + np.abs(lam)) + other)[ins], rows[ins])
    # P
    v1, vmax = float(v.sum()), float(v.max()) if len(v) else 0.0
    ok = v1 > feas_cert
    if kkt0 is not None:
        ok = ok and abs(vmax - kkt0) <= kkt0_atol
    out["P"] = dict(value=vmax, bound=float(kkt0) if kkt0 is not None else float("nan"), row=int(np.argmax(v)), ok=bool(ok), rows=int(iq.sum()), v1=v1)
    return out


def failed(res):
    """names of the residuals that are not within their bounds, in the order E S B V C P"""
    return [n for n in NAMES if not res[n]["ok"]]


class Worst:
    """running worst value of every residual over a set of certificates, for the tests' printed report"""

    def __init__(self):
        self.n = 0
        self.v = {n: 0.0 for n in NAMES[:5]}

    def add(self, res):
        self.n += 1
        for n in self.v:
            self.v[n] = max(self.v[n], res[n]["value"])

    def __str__(self):
        return "%d certificates; worst E %.1e  S %.1e  B (|lam| max) %.6g  V (rho - |lam|) %.1e  C (|lam| dist) %.1e" % (
            self.n, self.v["E"], self.v["S"], self.v["B"], self.v["V"], self.v["C"])


def srbm_certificate(O, x, p, lam, rho, tol, feas_cert=1e-4, kkt0=None, kkt0_atol=1e-9):
    """the SRBM NLP's data for certificate_residuals from the oracle: rows, bounds, and the sparse Jacobian (Oracle.jac_g in Oracle.pattern_jac)"""
    import scipy.sparse as sp
    x, p, lam = (np.ascontiguousarray(a, float) for a in (x, p, lam))
    g, jv = O.jac_g(x, p)
    ci, r = O.pattern_jac()
    J = sp.csc_matrix((jv, r, ci), shape=(O.ng, O.nx))
    lb, ub = O.bounds(p)
    return certificate_residuals(g, lb, ub, lam, rho, tol, J=J, feas_cert=feas_cert, kkt0=kkt0, kkt0_atol=kkt0_atol)


def kd_certificate(x, lam, lb, ub, N, dt, mass, Ib, Ibi, mu_fric, rho, tol, feas_cert=1e-4, kkt0=None, kkt0_atol=1e-9):
    """the kinodynamic refinement NLP's data for certificate_residuals from its oracle: rows from kinodyn_oracle.nlp_g_batch, J' lam from grad_lagrangian_batch with
    grad f = 0 (complex step, interval by interval), |J|' |lam| (the rounding allowance of S) from the complex-step Jacobian of kd_newton_reference, taken interval by interval"""
    import kd_newton_reference as kr
    from oracle import kinodyn_oracle as ko
    x, lam = np.asarray(x, float), np.asarray(lam, float)
    pr = kr.Problem(N, lb, ub, np.zeros(24), dt, mass, Ib, Ibi, mu_fric)
    g = pr.g(x)
    Jl = ko.grad_lagrangian_batch(x[None], lam[None], N, dt, mass, Ib, Ibi, mu_fric, np.zeros((1, pr.nx)))[0]
    aJ = np.asarray(abs(kr.jacobian_from_blocks(N, kr.jacobian_complex_step_blocks(pr, x))).T @ np.abs(lam)).ravel()
    return certificate_residuals(g, lb, ub, lam, rho, tol, Jt_lam=Jl, absJt_abslam=aJ, feas_cert=feas_cert, kkt0=kkt0, kkt0_atol=kkt0_atol)
