"""An independent reference for ONE Newton step of the kinodynamic refinement solver (landing_kd_head_kernel / landing_kd_condense_kernel /
landing_kd_iter_kernel, csrc/kd_solver_kernels.hip).  Test helper: numpy / scipy, oracle.kinodyn_oracle and the generic numerics of
tests/newton_reference.py (augmented and condensed assembly, extended-precision refinement, the yardsticks e_aug / e_cond, errors / bounds_of /
ratios / backward_error) -- this module only says what the system of THIS solver is:

  free variables   all of x but X_0 (x[0:12]) and c_0 (x[oU:oU+12], oU = 12 (N + 1) + 12 N).  Their step is prescribed, d sigma_0 = lb[0:24] - sigma_0, and
                   moves to the right-hand side (H_fc d sigma_0 to the stationarity rows, J_c d sigma_0 to the row residuals).
  rows             24 .. ng - 1.  Rows 0..23 fix sigma_0; rows 24..47 are one-sided copies of X_N (inequality rows); then 141 rows per interval (12 Euler
                   defects, 129 inequality rows), 117 in the last one.  The defects are the only equality rows.
  objective        the terminal cost: gradient 2 QN (X_N - ref), Hessian 2 diag(QN) on X_N;  H = that + Hessian of y' g, y = zU - zL on inequality rows.
  regularisation   delta on the diagonal of every stage block (kd_assemble_stage) and on X_N (kd_terminal): the feet c_1 .. c_{N-1} -- control of one
                   stage, state of the next -- receive 2 delta, every other free variable delta (d_reg; d_reg_plain is the delta * I the tests show to be wrong).

J and H are handed in by the caller (the complex-step Jacobian of the oracle's rows on the CPU; the product's function layer where the tests say so).

Intermediate quantities (sig_rho_reference, gc_reference) restate in np.longdouble what the kernels leave in the workspace: Sigma and rho of every row and, per
interval, the inequality rows' J_I' Sigma J_I (60 x 60) and J_I' rho (60) over v = (X_k, c_k, f_k, jpos_k, c_k+1) with the term sums that bound their rounding.
"""
import numpy as np
import scipy.sparse as sp

import conftest  # noqa: F401  (puts the repository root on sys.path: the oracle package)
import newton_reference as nr
from oracle import kinodyn_oracle as ko

LD = np.longdouble
EPS = float(np.finfo(float).eps)
BND, ROWS, ROWS_LAST, NW, NV = 48, 141, 117, 72, 60
GC = NV * NV + NV


class Problem:
    """one member: horizon, bounds, terminal cost data [QN | ref], step lengths and the model constants (mass, Ib, Ib_inv, friction mu)"""

    def __init__(self, N, lb, ub, cost, dt, mass, Ib, Ibi, mu_fric):
        self.N = N; self.lb = np.asarray(lb, float); self.ub = np.asarray(ub, float); self.cost = np.asarray(cost, float)
        self.dt = np.asarray(dt, float); self.mass = mass; self.Ib = np.asarray(Ib); self.Ibi = np.asarray(Ibi); self.mu_fric = mu_fric
        self.nx, self.ng = ko.nlp_dims(N)
        self.oU = 12 * (N + 1) + 12 * N

    def model(self):
        return self.dt, self.mass, self.Ib, self.Ibi, self.mu_fric

    def g(self, x):
        return ko.nlp_g_batch(np.asarray(x, float)[None], self.N, *self.model())[0]


def fixed_index(N):
    oU = 12 * (N + 1) + 12 * N
    return np.concatenate([np.arange(12), oU + np.arange(12)])


def free_index(N):
    return np.setdiff1d(np.arange(48 * N + 12), fixed_index(N))


def row_masks(pr):
    """(ineq, eq) over ng; asserts that the defects are the only equality rows behind the 24 rows that fix sigma_0"""
    rows = np.arange(pr.ng)
    eq = (pr.lb == pr.ub) & (rows >= 24)
    defect = np.zeros(pr.ng, bool)
    for k in range(pr.N):
        defect[BND + ROWS * k:BND + ROWS * k + 12] = True
    assert np.array_equal(eq, defect), "an equality row that is no Euler defect"
    assert (pr.lb[:24] == pr.ub[:24]).all()
    return (rows >= 24) & ~eq, eq


def foot_twice(N):
    """indices in x of the feet c_1 .. c_{N-1} (U_k = [c_k | f_k] at oU + 24 k)"""
    oU = 12 * (N + 1) + 12 * N
    return np.concatenate([oU + 24 * k + np.arange(12) for k in range(1, N)]) if N > 1 else np.zeros(0, int)


def d_reg(N, delta):
    d = np.full(48 * N + 12, float(delta))
    d[foot_twice(N)] *= 2.0
    return d


def d_reg_plain(N, delta):
    return np.full(48 * N + 12, float(delta))


def start_point(pr, x0):
    x = np.array(x0, float)
    x[0:12] = pr.lb[0:12]; x[pr.oU:pr.oU + 12] = pr.lb[12:24]
    return x


def initial_state(pr, x0, opts):
    """cold start (landing_kd_init_kernel restated): the callers' guess with X_0, c_0 from the bounds of rows 0..23, slacks pushed into the interior
    (newton_reference.push_slacks), multipliers of finite bounds 1.  opts carries explicit bound_push / bound_frac / mu_init."""
    x = start_point(pr, x0)
    s, zL, zU = nr.push_slacks(pr.g(x), pr.lb, pr.ub, opts.bound_push, opts.bound_frac, 24)
    return dict(x=x, s=s, zL=zL, zU=zU, y=zU - zL, mu=opts.mu_init)


# ---- J and H ---------------------------------------------------------------------------------------------------------------------------
def jacobian_complex_step(pr, x, h=1e-30, chunk=512):
    """dense [ng, nx]: the oracle's rows at x + i h e_j, all columns in one batched call (chunked only to bound the arrays): exact to rounding"""
    x = np.asarray(x, float)
    J = np.zeros((pr.ng, pr.nx))
    for lo in range(0, pr.nx, chunk):
        cols = np.arange(lo, min(lo + chunk, pr.nx))
        Xc = np.repeat(x[None].astype(complex), len(cols), axis=0)
        Xc[np.arange(len(cols)), cols] += 1j * h
        J[:, cols] = (ko.nlp_g_batch(Xc, pr.N, *pr.model()).imag / h).T
    return J


def w_map(N):
    return np.array([[ko.w_index(N, k, j) for j in range(NW)] for k in range(N)])


def boundary_jacobian(N):
    """rows 0..47: coordinate picks"""
    nx = 48 * N + 12; oU = 12 * (N + 1) + 12 * N
    r = np.arange(48)
    c = np.concatenate([np.arange(12), oU + np.arange(12), 12 * N + np.arange(6), 12 * N + np.arange(6), 12 * N + 6 + np.arange(6), 12 * N + 6 + np.arange(6)])
    return sp.csr_matrix((np.ones(48), (r, c)), shape=(48, nx))


def jacobian_from_blocks(N, Jb):
    """the function layer's blocks [N, 141, 72] (landing_kinodyn_nlp_eval) as the [ng, nx] Jacobian"""
    nx, ng = ko.nlp_dims(N)
    wm = w_map(N)
    rr, cc, vv = [], [], []
    for k in range(N):
        nrow = ROWS_LAST if k == N - 1 else ROWS
        on = wm[k] >= 0
        blk = np.asarray(Jb[k][:nrow])
        assert not blk[:, ~on].any()
        r, c = np.nonzero(blk[:, on])
        rr.append(BND + ROWS * k + r); cc.append(wm[k][on][c]); vv.append(blk[:, on][r, c])
    body = sp.csr_matrix((np.concatenate(vv), (np.concatenate(rr), np.concatenate(cc))), shape=(ng, nx))
    return (body + sp.vstack([boundary_jacobian(N), sp.csr_matrix((ng - 48, nx))])).tocsr()


def jacobian_complex_step_blocks(pr, x, h=1e-30):
    """the same derivative interval by interval (72 directions of the oracle's stage rows each), as blocks [N, 141, 72]: what the long horizons can afford"""
    x = np.asarray(x, float); N = pr.N
    wm = w_map(N)
    Jb = np.zeros((N, ROWS, NW))
    for k in range(N):
        W = np.where(wm[k] >= 0, x[np.maximum(wm[k], 0)], 0.0)
        Wc = np.repeat(W[None], NW, axis=0).astype(complex)
        Wc[np.arange(NW), np.arange(NW)] += 1j * h
        rows = ko.stage_rows_batch(Wc, np.full(NW, pr.dt[k]), k == N - 1, pr.mass, pr.Ib, pr.Ibi, pr.mu_fric)
        Jb[k, :rows.shape[1]] = (rows.imag / h).T
        Jb[k][:, wm[k] < 0] = 0.0
    return Jb


def hessian_from_blocks(N, Hb):
    """the function layer's blocks [N, 72, 72] of lam' g (landing_kinodyn_nlp_hess) summed into the sparse [nx, nx] Hessian (the boundary rows are linear)"""
    nx = 48 * N + 12
    wm = w_map(N)
    rr, cc, vv = [], [], []
    for k in range(N):
        blk = np.asarray(Hb[k])
        assert not blk[wm[k] < 0].any() and not blk[:, wm[k] < 0].any()
        r, c = np.nonzero(blk)
        rr.append(wm[k][r]); cc.append(wm[k][c]); vv.append(blk[r, c])
    return sp.csr_matrix((np.concatenate(vv), (np.concatenate(rr), np.concatenate(cc))), shape=(nx, nx))      # (duplicates are summed)


def hessian_check(pr, x, y, H, tol=1e-6, h=1e-5):
    """every column of H = Hessian of y' g against central differences of the oracle's grad_lagrangian_batch; returns the worst relative error"""
    x = np.asarray(x, float); nx = pr.nx
    H = H.toarray() if sp.issparse(H) else np.asarray(H)
    Xp = np.repeat(x[None], 2 * nx, axis=0)
    Xp[np.arange(nx), np.arange(nx)] += h; Xp[nx + np.arange(nx), np.arange(nx)] -= h
    gl = ko.grad_lagrangian_batch(Xp, np.repeat(np.asarray(y, float)[None], 2 * nx, axis=0), pr.N, *pr.model(), np.zeros((2 * nx, nx)))
    fd = ((gl[:nx] - gl[nx:]) / (2 * h)).T      # fd[:, j] = d (J' y) / d x_j
    worst = 0.0
    for j in range(nx):
        e = np.abs(H[:, j] - fd[:, j]).max() / max(1.0, np.abs(fd[:, j]).max())
        worst = max(worst, e)
        assert e <= tol, ("Hessian column", j, e)
    return worst


# ---- the step ---------------------------------------------------------------------------------------------------------------------------
def assemble(pr, st, mu, dreg, J, H):
    """the pieces of the step at st = dict(x, s, zL, zU, y) in the form newton_reference.solve_assembled takes; J [ng, nx], H [nx, nx] = Hessian of y' g"""
    N = pr.N
    ineq, eq = row_masks(pr)
    free, fixed, rows = free_index(N), fixed_index(N), np.arange(24, pr.ng)
    x = np.asarray(st["x"], float)
    J = sp.csr_matrix(J); Hf = sp.csr_matrix(H)
    qn = pr.cost[:12]; XN = slice(12 * N, 12 * N + 12)
    gf = np.zeros(pr.nx); gf[XN] = 2.0 * qn * (x[XN] - pr.cost[12:])
    Hobj = np.zeros(pr.nx); Hobj[XN] = 2.0 * qn
    Hf = (Hf + sp.diags(Hobj)).tocsr()
    d0 = np.concatenate([pr.lb[0:12] - x[0:12], pr.lb[12:24] - x[pr.oU:pr.oU + 12]])      # the prescribed step of sigma_0
    s, zL, zU = (np.asarray(st[k], float) for k in ("s", "zL", "zU"))
    sig, bar = nr.sigma_bar(s, zL, zU, pr.lb, pr.ub, mu, ineq)
    g = pr.g(x)      # (the oracle's rows, not the kernel's)
    res = np.where(ineq, g - s, g - pr.lb)
    Jr = J[rows]
    return dict(J=Jr[:, free], H=Hf[free][:, free], gf=gf[free] + Hf[free][:, fixed] @ d0, sig=sig[rows], bar=bar[rows], res=res[rows] + Jr[:, fixed] @ d0,
                ineq=ineq[rows], eq=eq[rows], D=np.asarray(dreg, float)[free], n=len(free), m=len(rows)), d0


def solve_step(pr, st, mu, dreg, J, H, refine=3):
    """refined Newton step at st (newton_reference.solve_assembled) over x / g: dict(dx, ds, y_new, ineq, eq, e_aug, e_cond, res, K, b, a, free, rows);
    dx of the fixed variables = their prescribed step, ds = J_I dx + (g - s) with it"""
    a, d0 = assemble(pr, st, mu, dreg, J, H)
    ref = nr.scatter(nr.solve_assembled(a, refine), pr.nx, pr.ng, free_index(pr.N), np.arange(24, pr.ng))
    ref["dx"][fixed_index(pr.N)] = d0
    return ref


# ---- intermediates ------------------------------------------------------------------------------------------------------------------------
def sig_rho_reference(pr, g, s, zL, zU, mu):
    """Sigma, rho = bar + Sigma (g - s) of every row in np.longdouble and the sums of the absolute values of their terms (kd_point_pass restated);
    zero on the rows without a slack"""
    ineq, _ = row_masks(pr)
    g, s, zL, zU, lb, ub = (np.asarray(v, LD) for v in (g, s, zL, zU, pr.lb, pr.ub))
    sig = np.zeros(pr.ng, LD); rho = np.zeros(pr.ng, LD); tsig = np.zeros(pr.ng, LD); trho = np.zeros(pr.ng, LD)
    hL = ineq & np.isfinite(pr.lb); hU = ineq & np.isfinite(pr.ub)
    mu = LD(mu)
    sig[hL] += zL[hL] / (s[hL] - lb[hL]); rho[hL] -= mu / (s[hL] - lb[hL]); trho[hL] += mu / (s[hL] - lb[hL])
    sig[hU] += zU[hU] / (ub[hU] - s[hU]); rho[hU] += mu / (ub[hU] - s[hU]); trho[hU] += mu / (ub[hU] - s[hU])
    tsig[:] = sig
    rho[ineq] += sig[ineq] * (g[ineq] - s[ineq]); trho[ineq] += np.abs(sig[ineq] * (g[ineq] - s[ineq]))
    return sig, rho, tsig, trho


def v_of_w():
    """block column w -> stage variable v (kd_v2w inverted); -1: the dropped columns 48..59 (X_k+1)"""
    return np.array([w if w < 48 else (-1 if w < 60 else w - 12) for w in range(NW)])


def gc_reference(N, J, sig, rho, rho_in_err=None):
    """Per interval k the inequality rows' G_k = J_I' Sigma J_I [60, 60] and m_k = J_I' rho [60] over v = (X_k, c_k, f_k, jpos_k, c_k+1), accumulated in
    np.longdouble over the non-zeros of J (the [ng, nx] Jacobian: the function layer's, not the solver's compact blocks), with the sums of the absolute values of the terms,
    and the worst number of terms of an entry.  Asserts that the inequality rows do not depend on X_k+1 (block columns 48..59).
    rho_in_err [ng]: a bound on the error of the rho the kernel used against the one given here; its share |J|' rho_in_err comes back as the last item.
    Returns (G [N, 60, 60], m [N, 60], absG, absm, most terms, input share of m [N, 60], terms per entry of G [N, 60, 60], of m [N, 60])."""
    wm = w_map(N); vw = v_of_w()
    J = sp.csr_matrix(J)
    sig = np.asarray(sig, LD); rho = np.asarray(rho, LD)
    G = np.zeros((N, NV, NV), LD); A = np.zeros((N, NV, NV), LD); m = np.zeros((N, NV), LD); Am = np.zeros((N, NV), LD); Em = np.zeros((N, NV), LD)
    most = 0
    nG = np.zeros((N, NV, NV), int); nm = np.zeros((N, NV), int)
    for k in range(N):
        nrow = ROWS_LAST if k == N - 1 else ROWS
        r0 = BND + ROWS * k + 12
        blk = J[r0:r0 + nrow - 12].tocoo()
        col2v = np.full(J.shape[1], -2)
        on = wm[k] >= 0
        col2v[wm[k][on]] = vw[on]
        v = col2v[blk.col]
        assert (v != -2).all(), ("an inequality row of interval %d depends on a variable outside its block" % k)
        assert not blk.data[v == -1].any(), ("an inequality row of interval %d depends on X_k+1" % k)
        keep = v >= 0
        r, v, val = blk.row[keep], v[keep], blk.data[keep].astype(LD)
        order = np.argsort(r, kind="stable"); r, v, val = r[order], v[order], val[order]
        cnt = np.bincount(r, minlength=nrow - 12); start = np.concatenate([[0], np.cumsum(cnt)])
        ia = np.repeat(np.arange(len(r)), cnt[r])                                  # every entry paired with every entry of its row
        ib = start[r[ia]] + (np.arange(len(ia)) - np.repeat(np.cumsum(cnt[r]) - cnt[r], cnt[r]))
        term = val[ia] * sig[r0 + r[ia]] * val[ib]
        np.add.at(G[k], (v[ia], v[ib]), term); np.add.at(A[k], (v[ia], v[ib]), np.abs(term))
        np.add.at(nG[k], (v[ia], v[ib]), 1); most = max(most, int(nG[k].max()))
        np.add.at(nm[k], v, 1)
        t = val * rho[r0 + r]
        np.add.at(m[k], v, t); np.add.at(Am[k], v, np.abs(t))
        if rho_in_err is not None:
            np.add.at(Em[k], v, np.abs(val) * np.asarray(rho_in_err, LD)[r0 + r])
    return G, m, A, Am, most, Em, nG, nm
