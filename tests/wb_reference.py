"""TEST INFRASTRUCTURE -- input laws, numpy references and the checks shared by tests/test_wb_kernels_cpu.py (the kernels through tests/emu)
and tests/test_gpu_wb_kernels.py (the product library) for the whole-body SQP kernels taken ONE AT A TIME: landing_wb_backward,
landing_wb_rollout (+ landing_wb_skip_taken), landing_wb_select, and the generic-tree path of landing_fb_dynamics_batch.

References: oracle/wb_oracle.py (dense Riccati recursion, rollout, cost) and oracle/rbd_oracle.py (6 x 6 Pluecker dynamics); for the backward pass
also one dense KKT solve of the whole LQ subproblem (kkt_lq below: no recursion, nothing shared with a Riccati sweep); for the selection a numpy
restatement of its rule (select_reference).  Every check function returns the figures it measured; the tests print them and assert the bounds."""
import ctypes as C
import functools

import numpy as np

from conftest import lc

# weights, step and step lengths of the rollout / loop tests (those of tests/test_wb.py)
DT = 0.001
Q = np.concatenate([np.full(3, 200.0), np.full(3, 100.0), np.full(12, 20.0), np.full(18, 0.5)])
R = np.full(12, 1e-3)
QN = 5.0 * Q
ALPHAS = (1.0, 0.5, 0.25, 0.1, 0.03)
SENTINEL = -7.25e300


# ---- where the arrays live: host arrays are the "device" memory of the emulation ---------------------------------------------------
class HostMem:
    stream = None

    def up(self, a, dtype=np.float64):
        return np.array(a, dtype=dtype, order="C")

    def ptr(self, a):
        return None if a is None else a.ctypes.data

    def down(self, a):
        return a.copy()


class CudaMem:
    def __init__(self):
        import torch
        self.t = torch

    @property
    def stream(self):
        return self.t.cuda.current_stream().cuda_stream

    def up(self, a, dtype=np.float64):
        return self.t.tensor(np.array(a, dtype=dtype, order="C"), device="cuda")

    def ptr(self, a):
        return None if a is None else a.data_ptr()

    def down(self, a):
        self.t.cuda.synchronize()
        return a.cpu().numpy()


class WbCalls:
    """the five whole-body entry points on numpy arrays (uploaded, called, read back), one context"""

    def __init__(self, L, mem, model=None):
        self.L, self.mem = L, mem
        self.rbd = lc("rbd").Rbd(L, model=model)

    def set_integrator(self, semi):
        self.L._check(self.L.lib.landing_wb_set_integrator(self.L.ctx, 1 if semi else 0), "landing_wb_set_integrator")

    @staticmethod
    def _w(*ws):
        keep = [np.ascontiguousarray(w, float) for w in ws]
        return keep, [k.ctypes.data_as(C.POINTER(C.c_double)) for k in keep]

    def backward(self, x, u, xref, A, Hinv, dt, reg, Qw, Rw, QNw):
        m = self.mem; B, N = u.shape[0], u.shape[1]
        d = [m.up(a) for a in (x, u, xref, A, Hinv)]
        K, kff, dV, ok = m.up(np.full((B, N, 12, 36), SENTINEL)), m.up(np.full((B, N, 12), SENTINEL)), m.up(np.full((B, 2), SENTINEL)), m.up(np.full(B, -9), np.int32)
        keep, w = self._w(Qw, Rw, QNw)
        self.L._check(self.L.lib.landing_wb_backward(self.L.ctx, B, N, dt, reg, *[m.ptr(a) for a in d], *w, m.ptr(K), m.ptr(kff), m.ptr(dV), m.ptr(ok), m.stream), "landing_wb_backward")
        return m.down(K), m.down(kff), m.down(dV), m.down(ok)

    def rollout(self, alphas, x, u, xref, f_foot, K, kff, dt, Qw, Rw, QNw, skip_step=None):
        """xnew / unew / cost are pre-filled with SENTINEL.  skip_step [B]: landing_wb_skip_taken with it just before the call"""
        m = self.mem; B, N = u.shape[0], u.shape[1]; na = len(alphas)
        al = m.up(alphas)
        d = [None if a is None else m.up(a) for a in (x, u, xref, f_foot, K, kff)]
        xn, un, cost = m.up(np.full((na, B, N + 1, 36), SENTINEL)), m.up(np.full((na, B, N, 12), SENTINEL)), m.up(np.full((na, B), SENTINEL))
        keep, w = self._w(Qw, Rw, QNw)
        st = None
        if skip_step is not None:
            st = m.up(skip_step)
            self.L._check(self.L.lib.landing_wb_skip_taken(self.L.ctx, m.ptr(st)), "landing_wb_skip_taken")
        self.L._check(self.L.lib.landing_wb_rollout(self.L.ctx, B, N, na, m.ptr(al), dt, *[m.ptr(a) for a in d], *w, m.ptr(xn), m.ptr(un), m.ptr(cost), m.stream), "landing_wb_rollout")
        out = m.down(xn), m.down(un), m.down(cost)
        del st
        return out

    def select(self, nalpha, alphas, ok, xnew, unew, costnew, x, u, cost, step):
        """nalpha < 0: keep mode.  Returns the updated (x, u, cost, step); step may be None (NULL)"""
        m = self.mem; B, N = u.shape[0], u.shape[1]
        al, dok = m.up(alphas), m.up(ok, np.int32)
        d = [m.up(a) for a in (xnew, unew, costnew, x, u, cost)]
        ds = None if step is None else m.up(step)
        self.L._check(self.L.lib.landing_wb_select(self.L.ctx, B, N, nalpha, m.ptr(al), m.ptr(dok), *[m.ptr(a) for a in d], m.ptr(ds), m.stream), "landing_wb_select")
        return m.down(d[3]), m.down(d[4]), m.down(d[5]), (None if ds is None else m.down(ds))

    def fb(self, q, qd, tau, f=None, want=("H", "C", "qdd", "A", "Hinv"), fd_h=0.0):
        m = self.mem; n = q.shape[0]
        shp = dict(H=(n, 18, 18), C=(n, 18), qdd=(n, 18), A=(n, 18, 36), Hinv=(n, 18, 18))
        o = {k: m.up(np.full(shp[k], SENTINEL)) for k in want}
        d = [None if a is None else m.up(a) for a in (q, qd, tau, f)]
        g = lambda k: m.ptr(o[k]) if k in o else 0
        self.rbd.fb_dynamics(n, m.ptr(d[0]), m.ptr(d[1]), m.ptr(d[2]) or 0, m.ptr(d[3]) or 0, g("H"), g("C"), g("qdd"), g("A"), g("Hinv"), fd_h, m.stream or 0)
        return {k: m.down(v) for k, v in o.items()}


def relerr(a, b):
    """max |a - b| relative to max |b|"""
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def relerr1(a, b):
    """max |a - b| relative to max(1, max |b|)"""
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b))))


# ==== 1. landing_wb_backward =========================================================================================================
def backward_inputs(rng, B, N):
    """synthetic stage data, not from the dynamics: A ~ N(0, 5^2), Hinv = 3 G G' + I, x / u / xref ~ N(0, 1), Q ~ U[0.5, 200], R ~ U[1e-3, 1e-1], QN ~ U[1, 500]"""
    A = 5.0 * rng.normal(size=(B * N, 18, 36))
    G = rng.normal(size=(B * N, 18, 18))
    Hinv = 3.0 * G @ np.swapaxes(G, 1, 2) + np.eye(18)
    x, u, xref = rng.normal(size=(B, N + 1, 36)), rng.normal(size=(B, N, 12)), rng.normal(size=(B, N + 1, 36))
    Qw, Rw, QNw = rng.uniform(0.5, 200.0, 36), rng.uniform(1e-3, 1e-1, 12), rng.uniform(1.0, 500.0, 36)
    return dict(A=A, Hinv=Hinv, x=x, u=u, xref=xref, Q=Qw, R=Rw, QN=QNw, dt=0.01, reg=0.0)


def kkt_lq(x, u, xref, Ads, Hinvs, dt, Qw, Rw, QNw, reg=0.0):
    """the LQ subproblem of one member as ONE dense KKT system over z = (dx_1 .. dx_N, du_0 .. du_N-1), dx_0 = 0:
         min  sum_k 1/2 dx_k' Q dx_k + (Q (x_k - xref_k))' dx_k + 1/2 du_k' (R + reg) du_k + (R u_k)' du_k  +  the same with QN at k = N
         s.t. dx_k+1 = A_k dx_k + B_k du_k.
    Returns du* [N, 12], dx* [N+1, 36] and the optimal value of the quadratic model.  Stage matrices by wb_oracle.stage_matrices (its SEMI switch)."""
    from oracle import wb_oracle as wo
    N = u.shape[0]; nx, nu = 36 * N, 12 * N; nz = nx + nu
    Hz = np.zeros((nz, nz)); g = np.zeros(nz); Gc = np.zeros((nx, nz))
    for k in range(1, N + 1):
        s = slice(36 * (k - 1), 36 * k)
        w = QNw if k == N else Qw
        Hz[s, s] = np.diag(w); g[s] = w * (x[k] - xref[k])
    for k in range(N):
        s = slice(nx + 12 * k, nx + 12 * (k + 1))
        Hz[s, s] = np.diag(Rw + reg); g[s] = Rw * u[k]
        Ak, Bk = wo.stage_matrices(Ads[k], Hinvs[k], dt)
        r = slice(36 * k, 36 * (k + 1))                       # row block: dx_k+1 - A_k dx_k - B_k du_k = 0
        Gc[r, r] = np.eye(36)
        if k > 0:
            Gc[r, 36 * (k - 1):36 * k] = -Ak
        Gc[r, s] = -Bk
    KKT = np.block([[Hz, Gc.T], [Gc, np.zeros((nx, nx))]])
    sol = np.linalg.solve(KKT, np.concatenate([-g, np.zeros(nx)]))
    z = sol[:nz]
    dx = np.concatenate([np.zeros((1, 36)), z[:nx].reshape(N, 36)]); du = z[nx:].reshape(N, 12)
    return du, dx, float(0.5 * z @ Hz @ z + g @ z)


def policy_rollout_linear(K, kff, Ads, Hinvs, dt):
    """du_k = kff_k + K_k dx_k on dx_k+1 = A_k dx_k + B_k du_k from dx_0 = 0"""
    from oracle import wb_oracle as wo
    N = kff.shape[0]; dx = np.zeros(36); du = np.zeros((N, 12))
    for k in range(N):
        Ak, Bk = wo.stage_matrices(Ads[k], Hinvs[k], dt)
        du[k] = kff[k] + K[k] @ dx
        dx = Ak @ dx + Bk @ du[k]
    return du


def check_backward(calls, N, B, semi, seed=0):
    """the kernel against (a) wb_oracle.lq_backward on the same stage matrices and (b) kkt_lq; returns the worst relative differences"""
    from oracle import wb_oracle as wo
    d = backward_inputs(np.random.default_rng(seed), B, N)
    calls.set_integrator(semi)
    K, kff, dV, ok = calls.backward(d["x"], d["u"], d["xref"], d["A"], d["Hinv"], d["dt"], d["reg"], d["Q"], d["R"], d["QN"])
    calls.set_integrator(False)
    assert (ok == 1).all(), ok
    fig = dict(K=0.0, kff=0.0, dV=0.0, du=0.0, value=0.0, half=0.0, oracle_du=0.0, oracle_value=0.0)
    wo.SEMI = semi
    try:
        for b in range(B):
            Ab, Hb = d["A"][b * N:(b + 1) * N], d["Hinv"][b * N:(b + 1) * N]
            Ko, ko, dVo = wo.lq_backward(d["x"][b], d["u"][b], d["xref"][b], Ab, Hb, d["dt"], d["Q"], d["R"], d["QN"], d["reg"])
            du_s, _, val = kkt_lq(d["x"][b], d["u"][b], d["xref"][b], Ab, Hb, d["dt"], d["Q"], d["R"], d["QN"], d["reg"])
            du_k = policy_rollout_linear(K[b], kff[b], Ab, Hb, d["dt"])
            du_o = policy_rollout_linear(Ko, ko, Ab, Hb, d["dt"])
            new = dict(K=relerr(K[b], Ko), kff=relerr(kff[b], ko), dV=relerr(dV[b], dVo), du=relerr(du_k, du_s), value=abs(dV[b, 0] + dV[b, 1] - val) / abs(val),
                       half=abs(dV[b, 1] + 0.5 * dV[b, 0]) / abs(dV[b, 0]), oracle_du=relerr(du_o, du_s), oracle_value=abs(dVo[0] + dVo[1] - val) / abs(val))
            fig = {k: max(fig[k], new[k]) for k in fig}
    finally:
        wo.SEMI = False
    return fig


def backward_branch_inputs(N=3, B=4, singular=2, scale=40.0, seed=1):
    """a batch whose member `singular` has Hinv = 0 under reg = -2 min(R): its Quu = diag(R) + reg has a negative entry.  The other members' Hinv is scaled
    so that B' V B outweighs reg"""
    d = backward_inputs(np.random.default_rng(seed), B, N)
    d["Hinv"] = d["Hinv"] * scale
    d["Hinv"][singular * N:(singular + 1) * N] = 0.0
    d["reg"] = -2.0 * float(d["R"].min())
    return d


def oracle_quu_min_eig(d, b, semi):
    from oracle import wb_oracle as wo
    N = d["u"].shape[1]; quu = []
    wo.SEMI = semi
    try:
        wo.lq_backward(d["x"][b], d["u"][b], d["xref"][b], d["A"][b * N:(b + 1) * N], d["Hinv"][b * N:(b + 1) * N], d["dt"], d["Q"], d["R"], d["QN"], d["reg"], quu_out=quu)
    finally:
        wo.SEMI = False
    return min(float(np.linalg.eigvalsh(0.5 * (m + m.T)).min()) for m in quu)


def check_backward_branches(calls, semi):
    """ok = 0 with finite outputs for the singular member; every other member bit-identical to a call on it alone, and equal to the oracle"""
    from oracle import wb_oracle as wo
    N, B, sing = 3, 4, 2
    d = backward_branch_inputs(N, B, sing)
    calls.set_integrator(semi)
    args = lambda s: (d["x"][s], d["u"][s], d["xref"][s], d["A"][s.start * N:s.stop * N], d["Hinv"][s.start * N:s.stop * N], d["dt"], d["reg"], d["Q"], d["R"], d["QN"])
    K, kff, dV, ok = calls.backward(*args(slice(0, B)))
    worst = 0.0
    for b in range(B):
        K1, k1, dV1, ok1 = calls.backward(*args(slice(b, b + 1)))
        assert np.array_equal(K[b], K1[0]) and np.array_equal(kff[b], k1[0]) and np.array_equal(dV[b], dV1[0]) and ok[b] == ok1[0], b
        if b == sing:
            assert ok[b] == 0 and np.isfinite(K[b]).all() and np.isfinite(kff[b]).all() and np.isfinite(dV[b]).all()
            continue
        assert ok[b] == 1
        assert oracle_quu_min_eig(d, b, semi) > 0.0
        wo.SEMI = semi
        try:
            Ko, ko, dVo = wo.lq_backward(d["x"][b], d["u"][b], d["xref"][b], d["A"][b * N:(b + 1) * N], d["Hinv"][b * N:(b + 1) * N], d["dt"], d["Q"], d["R"], d["QN"], d["reg"])
        finally:
            wo.SEMI = False
        worst = max(worst, relerr(K[b], Ko), relerr(kff[b], ko), relerr(dV[b], dVo))
    calls.set_integrator(False)
    return worst


# ==== 2. landing_wb_rollout ==========================================================================================================
def points(rng, n):
    """tests/test_rbd.py::_points with the velocities scaled by 0.3"""
    q = np.zeros((n, 18)); qd = 0.3 * rng.normal(size=(n, 18)); tau = 5 * rng.normal(size=(n, 18)); f = np.zeros((n, 12))
    for i in range(n):
        q[i, :3] = [rng.normal() * 0.3, rng.normal() * 0.3, 0.3 + 0.2 * rng.random()]
        q[i, 3:6] = 0.5 * rng.normal(size=3)
        q[i, 6:] = np.tile([0.0, -0.8, 1.6], 4) + 0.3 * rng.normal(size=12)
        f[i] = np.tile([3.0, -2.0, 25.0], 4) + 6 * rng.normal(size=12)
    return q, qd, tau, f


@functools.lru_cache(maxsize=None)
def rollout_inputs(B, N, seed=3):
    """the nominal trajectory's knots, the reference and the forces are independent points; K ~ 0.5 N(0, 1), kff ~ N(0, 1)"""
    rng = np.random.default_rng(seed)
    q, qd, tau, f = points(rng, B * (N + 1))
    x = np.concatenate([q, qd], axis=1).reshape(B, N + 1, 36)
    q2, qd2, _, _ = points(rng, B * (N + 1))
    xref = np.concatenate([q2, qd2], axis=1).reshape(B, N + 1, 36)
    u = tau[:B * N, 6:].reshape(B, N, 12).copy(); ff = f[:B * N].reshape(B, N, 12).copy()
    K = 0.5 * rng.normal(size=(B, N, 12, 36)); kff = rng.normal(size=(B, N, 12))
    out = dict(x=x, u=u, xref=xref, f=ff, K=K, kff=kff)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rollout_oracle(nalpha, B, N, with_f, semi, closed, seed=3):
    """wb_oracle.rollout / cost_of for every (ia, b) slot (computed once per case, shared by the tests; read-only)"""
    from oracle import wb_oracle as wo
    d = rollout_inputs(B, N, seed)
    xs, us, cs = np.zeros((nalpha, B, N + 1, 36)), np.zeros((nalpha, B, N, 12)), np.zeros((nalpha, B))
    wo.SEMI = semi
    try:
        for ia in range(nalpha):
            for b in range(B):
                xs[ia, b], us[ia, b] = wo.rollout(d["x"][b, 0], d["u"][b], d["x"][b], d["K"][b] if closed else None, d["kff"][b] if closed else None, ALPHAS[ia],
                                                  d["f"][b] if with_f else None, DT)
                cs[ia, b] = wo.cost_of(xs[ia, b], us[ia, b], d["xref"][b], Q, R, QN)
    finally:
        wo.SEMI = False
    for v in (xs, us, cs):
        v.setflags(write=False)
    return xs, us, cs


PERM = np.array([0, 1, 2, 3, 4, 5, 6, 9, 12, 15, 7, 10, 13, 16, 8, 11, 14, 17])      # new body i is old body PERM[i]: the leg bodies joint-type-major
PERM_X = np.concatenate([PERM, 18 + PERM]); PERM_U = PERM[6:] - 6


def permuted_model():
    """the quadruped with its twelve leg bodies renumbered joint-type-major: a valid tree that is NOT the arrow topology, and whose legs are not consecutive bodies"""
    rbd = lc("rbd")
    S, M = rbd.quad3d_model(), rbd.RbdModel()
    parent = [0, 1, 2, 3, 4, 5, 6, 6, 6, 6, 7, 8, 9, 10, 11, 12, 13, 14]
    for i, o in enumerate(PERM):
        M.parent[i] = parent[i]; M.jtype[i] = S.jtype[o]; M.m[i] = S.m[o]
        for j in range(9): M.E[i][j] = S.E[o][j]
        for j in range(3): M.r[i][j] = S.r[o][j]; M.h[i][j] = S.h[o][j]
        for j in range(6): M.I[i][j] = S.I[o][j]
    for leg in range(4):
        M.b_foot[leg] = 15 + leg
        for j in range(3): M.foot_r[leg][j] = S.foot_r[leg][j]
    M.l1, M.l2, M.l3, M.l4 = S.l1, S.l2, S.l3, S.l4
    return M


def check_rollout(calls, nalpha, B, N, with_f, semi, closed, permuted=False):
    """every (ia, b) slot of xnew / unew / cost against the oracle, relative to max(1, |.|).  permuted: `calls` holds permuted_model(); the inputs are
    handed over in its numbering and the outputs brought back"""
    d = rollout_inputs(B, N)
    xo, uo, co = rollout_oracle(nalpha, B, N, with_f, semi, closed)
    px, pu = (PERM_X, PERM_U) if permuted else (np.arange(36), np.arange(12))
    calls.set_integrator(semi)
    xn, un, cn = calls.rollout(ALPHAS[:nalpha], d["x"][..., px], d["u"][..., pu], d["xref"][..., px], d["f"] if with_f else None,
                               d["K"][..., pu, :][..., px] if closed else None, d["kff"][..., pu] if closed else None, DT, Q[px], R[pu], QN[px])
    calls.set_integrator(False)
    ix, iu = np.argsort(px), np.argsort(pu)
    xn, un = xn[..., ix], un[..., iu]
    return dict(x=relerr1(xn, xo), u=relerr1(un, uo), cost=max(abs(cn[i, b] - co[i, b]) / max(1.0, abs(co[i, b])) for i in range(nalpha) for b in range(B)))


def check_rollout_skip(calls, with_f=True):
    """landing_wb_skip_taken: masked members get cost = +inf and keep the sentinel, the others equal an unmasked call bit for bit; the mask is consumed once"""
    nalpha, B, N = 3, 7, 4
    d = rollout_inputs(B, N)
    a = (ALPHAS[:nalpha], d["x"], d["u"], d["xref"], d["f"] if with_f else None, d["K"], d["kff"], DT, Q, R, QN)
    step = np.array([0.0, 1.0, 0.0, 0.5, 0.0, 0.0, 0.03])
    x0, u0, c0 = calls.rollout(*a)
    assert np.isfinite(c0).all() and not (x0 == SENTINEL).any() and not (u0 == SENTINEL).any()
    x1, u1, c1 = calls.rollout(*a, skip_step=step)
    for b in range(B):
        if step[b] != 0.0:
            assert (c1[:, b] == np.inf).all() and (x1[:, b] == SENTINEL).all() and (u1[:, b] == SENTINEL).all(), b
        else:
            assert np.array_equal(x1[:, b], x0[:, b]) and np.array_equal(u1[:, b], u0[:, b]) and np.array_equal(c1[:, b], c0[:, b]), b
    x2, u2, c2 = calls.rollout(*a)      # no new landing_wb_skip_taken: everybody again
    assert np.array_equal(x2, x0) and np.array_equal(u2, u0) and np.array_equal(c2, c0)


def check_rollout_header_claim(calls, with_f, n=6):
    """N = 1: the rollout's velocity update against dt qdd of landing_fb_dynamics_batch (the hand_c / chol_solve18 kernels).  Returns the worst difference
    relative to max(1, |dt qdd|) and whether qd + dt qdd reproduces the rollout's velocities bit for bit"""
    d = rollout_inputs(n, 1)
    x, u, f = d["x"], d["u"], (d["f"] if with_f else None)
    xn, _, _ = calls.rollout((1.0,), x, u, d["xref"], f, None, None, DT, Q, R, QN)
    tau = np.concatenate([np.zeros((n, 6)), u[:, 0]], axis=1)
    qdd = calls.fb(x[:, 0, :18].copy(), x[:, 0, 18:].copy(), tau, f[:, 0].copy() if with_f else None, want=("qdd",), fd_h=1e-6)["qdd"]
    lhs = xn[0, :, 1, 18:] - x[:, 0, 18:]
    return relerr1(lhs, DT * qdd), bool(np.array_equal(x[:, 0, 18:] + DT * qdd, xn[0, :, 1, 18:]))


# ==== 3. landing_wb_select ===========================================================================================================
def select_reference(nalpha, keep, alphas, ok, xnew, unew, costnew, x, u, cost, step):
    """member b takes the FIRST entry whose cost is strictly below its own, unless ok[b] = 0 or (keep mode) its step is already non-zero; step = the alpha taken or 0"""
    x, u, cost = x.copy(), u.copy(), cost.copy(); step = None if step is None else step.copy()
    for b in range(cost.shape[0]):
        taken = keep and step is not None and step[b] != 0.0
        pick = -1
        if ok[b] and not taken:
            for ia in range(nalpha):
                if costnew[ia, b] < cost[b]:
                    pick = ia
                    break
        if pick >= 0:
            x[b], u[b], cost[b] = xnew[pick, b], unew[pick, b], costnew[pick, b]
        if step is not None and not taken:
            step[b] = alphas[pick] if pick >= 0 else 0.0
    return x, u, cost, step


def select_case(N, nalpha, seed=0):
    """B = 7 members: first entry wins | last entry wins | no improvement | a cost EQUAL to the current one (not taken) | +inf before a winner | ok = 0 |
    an ordinary member with two improving entries (the first is taken, not the best)"""
    rng = np.random.default_rng(seed)
    B = 7
    cost = rng.uniform(5.0, 10.0, B)
    cn = cost[None, :] + rng.uniform(0.5, 2.0, (nalpha, B))           # nothing improves ...
    cn[0, 0] = cost[0] - 1.0                                          # ... member 0: the first entry
    cn[nalpha - 1, 1] = cost[1] - 1.0                                 # member 1: the last entry only
    cn[:, 3] = cost[3]                                                # member 3: equal costs everywhere
    cn[:nalpha - 1, 4] = np.inf; cn[nalpha - 1, 4] = cost[4] - 2.0    # member 4: +inf, then a winner (nalpha = 1: the winner alone)
    cn[:, 5] = cost[5] - 3.0                                          # member 5: would improve, but ok = 0
    cn[0, 6] = cost[6] - 0.5; cn[nalpha - 1, 6] = cost[6] - (1.0 if nalpha > 1 else 0.5)
    ok = np.ones(B, np.int32); ok[5] = 0
    xnew, unew = rng.normal(size=(nalpha, B, N + 1, 36)), rng.normal(size=(nalpha, B, N, 12))
    x, u = rng.normal(size=(B, N + 1, 36)), rng.normal(size=(B, N, 12))
    alphas = np.array([1.0, 0.5, 0.25, 0.1][:nalpha])
    return dict(alphas=alphas, ok=ok, xnew=xnew, unew=unew, costnew=cn, x=x, u=u, cost=cost)


def check_select(calls, N, nalpha):
    c = select_case(N, nalpha)
    a = (c["alphas"], c["ok"], c["xnew"], c["unew"], c["costnew"], c["x"], c["u"], c["cost"])
    eq = lambda got, want: all((g is None and w is None) or np.array_equal(g, w) for g, w in zip(got, want))
    # search mode, with and without a step array
    for step in (np.full(7, SENTINEL), None):
        got = calls.select(nalpha, *a, step)
        want = select_reference(nalpha, False, *a, step)
        assert eq(got, want), (N, nalpha, "search", got[3], want[3])
    want_step = select_reference(nalpha, False, *a, np.zeros(7))[3]
    assert want_step[0] == c["alphas"][0] and want_step[1] == c["alphas"][-1] and want_step[4] == c["alphas"][-1] and (want_step[[2, 3, 5]] == 0).all() and want_step[6] == c["alphas"][0]
    # keep mode: members 0, 2 and 4 already hold a step (member 2 would not improve anyway, 0 and 4 would): they keep everything, the others are searched
    step = np.zeros(7); step[[0, 2, 4]] = [1.0, 0.25, 0.03]
    got = calls.select(-nalpha, *a, step)
    want = select_reference(nalpha, True, *a, step)
    assert eq(got, want), (N, nalpha, "keep", got[3], want[3])
    for b in (0, 2, 4):
        assert np.array_equal(got[0][b], c["x"][b]) and np.array_equal(got[1][b], c["u"][b]) and got[2][b] == c["cost"][b] and got[3][b] == step[b]
    assert got[3][1] == c["alphas"][-1] and np.array_equal(got[0][1], c["xnew"][nalpha - 1, 1])
    # keep mode with nothing taken yet == search mode
    assert eq(calls.select(-nalpha, *a, np.zeros(7)), select_reference(nalpha, False, *a, np.zeros(7)))


def check_select_argument_errors(calls):
    import pytest
    c = select_case(3, 1)
    a = (c["alphas"], c["ok"], c["xnew"], c["unew"], c["costnew"], c["x"], c["u"], c["cost"])
    with pytest.raises(RuntimeError, match="landing_wb_select"):
        calls.select(0, *a, np.zeros(7))
    with pytest.raises(RuntimeError, match="landing_wb_select"):
        calls.select(-1, *a, None)


# ==== 4. the loop when it backtracks =================================================================================================
# (step lengths, semi-implicit): the two lists of the issue, and MIXED -- found by a search over first entries around 2 on the emulation -- in whose
# iterations members of ONE batch take different entries, some the first (stage 1 of the fused search) and some a later one (stage 2)
LOOP_SEED, LOOP_B, LOOP_N, LOOP_ITERS = 5, 6, 5, 3
LOOP_LISTS = {"a": (2.5, 2.0, 1.5, 1.0), "b": (3.0, 2.2, 1.9, 1.0, 0.5), "mixed": (1.9946, 1.5, 1.0)}
# "mixed": the cost model's threshold is alpha = 2; at the first iteration the members' own thresholds lie between 1.99443 and 1.99477 (probed in steps of 1e-4 on the
# emulation), so with 1.9946 member 5 takes the first entry (its cost falls by 3.7e-5 relative) and members 0..4 miss it by 1.3e-5 .. 6e-5 relative and take 1.5 in the
# second stage -- margins four orders above the 1e-9 to which the two sides' costs agree.  Every other decision of the three lists has a margin of 4e-4 or more.
LOOP_CASES = (("a", False), ("b", False), ("mixed", False), ("a", True))      # (list, semi-implicit): what tests/golden/wb_backtrack.npz holds
LOOP_GOLDEN = "wb_backtrack.npz"


def loop_golden(golden_dir, name, semi):
    """the oracle's (alphas [iters, B], cost history [iters + 1, B]) as recorded by tests/make_golden_wb.py"""
    import os
    z = np.load(os.path.join(golden_dir, LOOP_GOLDEN))
    key = "%s_%s" % (name, "semi" if semi else "expl")
    return z[key + "_alpha"], z[key + "_cost"]


def loop_problem():
    import test_wb
    return test_wb._problem(np.random.default_rng(LOOP_SEED), LOOP_B, LOOP_N)


def loop_oracle(alphas, semi):
    """wb_oracle.solve for every member: alphas [iters, B], cost history [iters + 1, B]"""
    import test_wb
    from oracle import wb_oracle as wo
    x0, u0, xref, f = loop_problem()
    al, hist = np.zeros((LOOP_ITERS, LOOP_B)), np.zeros((LOOP_ITERS + 1, LOOP_B))
    wo.SEMI = semi
    try:
        for b in range(LOOP_B):
            _, _, hist[:, b], al[:, b] = wo.solve(x0[b], u0[b], xref[b], f[b], test_wb.DT, test_wb.Q, test_wb.R, test_wb.QN, LOOP_ITERS, alphas=alphas, K_init=test_wb.KPD,
                                                  return_alphas=True)
    finally:
        wo.SEMI = False
    return al, hist


def loop_run(L, dev, alphas, semi, fused):
    import torch
    import test_wb
    x0, u0, xref, f = loop_problem()
    S = lc("wb").WholeBodySQP(L, lc("rbd").Rbd(L), LOOP_N, test_wb.DT, test_wb.Q, test_wb.R, test_wb.QN, device=dev, alphas=alphas, semi_implicit=semi, fused=fused)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    out = S.solve(t(x0), t(u0), t(xref), t(f), iters=LOOP_ITERS, K_init=test_wb.KPD)
    lc("wb").WholeBodySQP(L, S.R_, LOOP_N, test_wb.DT, test_wb.Q, test_wb.R, test_wb.QN, device=dev)      # (the context's integrator back to explicit)
    return {k: out[k].cpu().numpy() for k in ("alpha", "cost", "x", "u", "expected")}


# ==== 5. the generic-tree path =======================================================================================================
def check_generic_tree(calls_perm, calls_std, npts, n_fd, seed=3):
    """landing_fb_dynamics_batch on permuted_model() (generic recursion, dense solve) against the oracle evaluated at the un-permuted points, and its exact A
    against the quad path's on the standard model.  n_fd: how many points get the oracle's (slow) Richardson and central-difference Jacobians.
    Returns the worst figures, each relative as tests/test_rbd.py measures it"""
    from oracle import rbd_oracle as ro
    q, qd, tau, _ = points(np.random.default_rng(seed), npts)
    P = PERM
    o = calls_perm.fb(q[:, P], qd[:, P], tau[:, P], None, fd_h=0.0)
    ofd = calls_perm.fb(q[:, P], qd[:, P], tau[:, P], None, want=("qdd", "A"), fd_h=1e-6)
    s = calls_std.fb(q, qd, tau, None, want=("A",), fd_h=0.0)
    assert not any((v == SENTINEL).any() for v in list(o.values()) + list(ofd.values()) + list(s.values()))
    fig = dict(H=0.0, C=0.0, qdd=0.0, qdd_fd=0.0, Hinv=0.0, A_richardson=0.0, A_fd=0.0, A_quad=0.0)
    for i in range(npts):
        Ho, Co = ro.hand_c(q[i], qd[i], None)
        qo = np.linalg.solve(Ho, tau[i] - Co); Hio = np.linalg.inv(Ho)
        new = dict(H=relerr(o["H"][i], Ho[np.ix_(P, P)]), C=relerr1(o["C"][i], Co[P]), qdd=relerr1(o["qdd"][i], qo[P]), qdd_fd=relerr1(ofd["qdd"][i], qo[P]),
                   Hinv=relerr(o["Hinv"][i], Hio[np.ix_(P, P)]), A_quad=relerr1(o["A"][i], s["A"][i][np.ix_(P, PERM_X)]))
        if i < n_fd:
            new["A_richardson"] = relerr1(o["A"][i], ro.richardson_linearisation(q[i], qd[i], tau[i], None)[np.ix_(P, PERM_X)])
            new["A_fd"] = relerr1(ofd["A"][i], ro.fd_linearisation(q[i], qd[i], tau[i], None, h=1e-6)[1][np.ix_(P, PERM_X)])
        fig = {k: max(fig[k], new.get(k, 0.0)) for k in fig}
    return fig


GENERIC_BOUNDS = dict(H=1e-11, C=1e-11, qdd=1e-9, qdd_fd=1e-9, Hinv=1e-9, A_richardson=1e-8, A_fd=1e-5, A_quad=1e-12)      # tests/test_rbd.py's; A_quad: the issue's
